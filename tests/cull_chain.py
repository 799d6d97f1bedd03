"""The tail of a mapping cycle as ONE captured graph, for tests/test_gpu_keyframe_culling_chain.py.  Four calls on one stream,
nothing read back in between:
  spfe_count_observations_resident (d_mp_nobs from the rows) -> spfe_cull_keyframes_resident (the covisible keyframes of keyframe
  K - 1) -> spfe_update_connections_resident (the NEXT keyframe, K, on the rows, flags and graph the cull left) ->
  spfe_update_local_map_resident (its 20-column table and d_parent from the graph state, d_kf_flags with the cull's new bits)
against the host references chained in Python (tests/cull_ref, tests/covis_ref, tests/localmap_ref).

    python -m tests.cull_chain      the graph captured once on input A and replayed on A, on B and on A again (one fresh process,
                                    one verdict line).  The process's hardware queue count is left as the machine sets it.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "cull_ref", "covis_ref", "localmap_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
sys.path.insert(0, ROOT)
import covis_ref  # noqa: E402
import cull_cases as cc  # noqa: E402
import cull_ref  # noqa: E402
import localmap_ref  # noqa: E402

N_SLOTS, K, HOLD, TH, TH_OBS, COV_RATIO, BAD_CAP, POINT_CAP, FILL = 48, 30, 4, 4, 3, 0.5, 20, 512, 0xA5
N_BEST_A, N_BEST_B = 20, 10
BLOCKS = ("d_cull_out", "d_covis_out", "d_lm_out")
LAUNCHES = 2 + 4 + 5 + 7       # the count, the cull, UpdateConnections, the local map
PRM = dict(cur=K - 1, th_obs=TH_OBS, cov_ratio=COV_RATIO, origin_slot=0, bad_cap=BAD_CAP)


def build_world(refs, seed):
    """the map as K keyframes left it — each inserted and connected, and all but the last HOLD culled around, by the references —, one
    listed keyframe marked not-erase, and the row of keyframe K appended for the insertion that follows the cull"""
    rk, rc, _ = refs
    w, rng, geo = cc.sequence_world(seed, n_slots=N_SLOTS)
    for s in range(K):
        cc.insert_keyframe(w, rng, geo, s)
        covis_ref.update(rc, w["rows"], w["kf_flags"], w["mp_flags"], {k: w[k] for k in covis_ref.STATE}, s, TH, 0, w["best_a"], w["best_b"])
        if s < K - HOLD:                                   # the last few stay for the chain's cull
            cull_ref.cull(rk, w, **dict(PRM, cur=s))
    listed = w["ord_slot"][K - 1, :w["ord_n"][K - 1]]
    w["kf_flags"][listed[len(listed) // 2]] |= cull_ref.KF_NOT_ERASE
    cc.insert_keyframe(w, rng, geo, K)
    w["nobs"][:] = -77                                     # the count's work
    return w


def chain(e, P, graph, stride, n_table, stream):
    """the four calls on the addresses P[name], on `stream`: nothing is read back, no tensor is made"""
    e.count_observations_resident(P["rows"], stride, P["kf_flags"], N_SLOTS, P["nobs"], n_table, stream=stream)
    e.cull_keyframes_resident(graph, P["rows"], stride, P["kf_flags"], P["mp_flags"], P["nobs"], n_table, K - 1, P["d_cull_out"],
                              th_obs=TH_OBS, cov_ratio=COV_RATIO, origin_slot=0, bad_cap=BAD_CAP, d_best_cov_a=P["best_a"],
                              n_best_a=N_BEST_A, d_best_cov_b=P["best_b"], n_best_b=N_BEST_B, stream=stream)
    e.update_connections_resident(graph, P["rows"], stride, P["kf_flags"], P["mp_flags"], n_table, K, P["d_covis_out"], th=TH,
                                  origin_slot=0, d_best_cov_a=P["best_a"], n_best_a=N_BEST_A, d_best_cov_b=P["best_b"],
                                  n_best_b=N_BEST_B, stream=stream)
    e.update_local_map_resident(P["rows"], stride, P["kf_flags"], P["best_a"], N_BEST_A, P["parent"], N_SLOTS, P["mp_flags"], n_table,
                                P["rows"] + 4 * K * stride, stride, P["d_lm_out"], POINT_CAP, stream=stream)


def host_route(refs, world):
    """the same four steps through the host references on a copy -> (the world after, the three blocks, their decoded forms)"""
    rk, rc, rm = refs
    w = cull_ref.copy_world(world)
    w["nobs"][:] = cull_ref.count(rk, w["rows"], w["kf_flags"], len(w["mp_flags"]))
    k = cull_ref.cull(rk, w, **PRM)
    c = covis_ref.update(rc, w["rows"], w["kf_flags"], w["mp_flags"], {s: w[s] for s in covis_ref.STATE}, K, TH, 0, w["best_a"], w["best_b"])
    m = localmap_ref.update(rm, dict(kf_mp_of_kp=w["rows"], kf_flags=w["kf_flags"], best_cov=w["best_a"], parent=w["parent"],
                                     mp_flags=w["mp_flags"], mp_of_kp=w["rows"][K], max_keyframes=80, point_cap=POINT_CAP))
    return w, dict(d_cull_out=k["block"], d_covis_out=c["block"], d_lm_out=m["block"]), dict(cull=k, covis=c, lm=m)


def main():
    import torch
    import hip_graph
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    e = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    tmp = tempfile.mkdtemp(prefix="cull_chain_")
    refs = (cull_ref.build(tmp), covis_ref.build(tmp), localmap_ref.build(tmp))
    worlds = {"A": build_world(refs, 801), "B": build_world(refs, 802)}
    n, stride = worlds["A"]["rows"].shape
    n_table, cap = len(worlds["A"]["mp_flags"]), worlds["A"]["conn_slot"].shape[1]
    raw = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint8)   # noqa: E731
    size = {k: len(raw(v)) for k, v in worlds["A"].items()}
    size.update(d_cull_out=e.cull_out_bytes(n, cap, BAD_CAP), d_covis_out=e.covis_out_bytes(n, cap),
                d_lm_out=e.localmap_out_bytes(n, POINT_CAP, stride))
    bufs = {k: torch.full((sz + 16,), FILL, dtype=torch.uint8, device="cuda") for k, sz in size.items()}
    P = {k: t.data_ptr() for k, t in bufs.items()}
    graph = X.covis_graph({k: P[k] for k in cull_ref.STATE}, n, cap)
    img = {key: {k: torch.from_numpy(raw(v).copy()) for k, v in w.items()} for key, w in worlds.items()}
    stream = torch.cuda.Stream()

    def load(key):
        for k in size:
            if k in img[key]:
                bufs[k][:size[k]].copy_(img[key][k])
            else:
                bufs[k].fill_(FILL)
        torch.cuda.synchronize()

    def read():
        torch.cuda.synchronize()
        return {k: bufs[k][:size[k]].cpu().numpy() for k in size}

    want, info = {}, {}
    for key, w in worlds.items():
        after, blocks, info[key] = host_route(refs, w)
        want[key] = {k: raw(after[k]).copy() for k in cull_ref.WORLD}
        want[key].update(blocks)

    def differences(got, key, what):
        return ["%s: %r differs from the host references in %d byte(s), the first at %d" % (
            what, k, (got[k] != want[key][k]).sum(), np.flatnonzero(got[k] != want[key][k])[0])
            for k in size if (got[k] != want[key][k]).any()]

    failures = []
    for key in ("A", "B"):                # direct calls first: they size the handle's scratch, the only size there is
        load(key)
        chain(e, P, graph, stride, n_table, stream.cuda_stream)
        failures += differences(read(), key, "direct chain on %s" % key)
        h = info[key]
        print("%s: culled %s deferred %d bad points %d touched %d events %d | keyframe %d linked %d parent %d | local keyframes %d points %d"
              % (key, h["cull"]["culled_slot"][:h["cull"]["n_culled"]].tolist(), h["cull"]["n_deferred"], h["cull"]["n_bad"],
                 h["cull"]["n_touched"], h["cull"]["n_events"], K, h["covis"]["n_linked"], h["covis"]["parent_set"],
                 h["lm"]["n_local_kf"], h["lm"]["n_points"]))
        if not (h["cull"]["n_culled"] >= 1 and h["cull"]["n_touched"] >= 1 and h["covis"]["status"] == 0 and h["covis"]["n_linked"] >= 2
                and h["covis"]["parent_set"] >= 0 and h["lm"]["n_local_kf"] >= 2 and h["lm"]["n_points"] > stride // 2):
            failures.append("%s: the case does not exercise the chain" % key)
    if any(want["A"][k].tobytes() == want["B"][k].tobytes() for k in BLOCKS):
        failures.append("A and B give the same block: the replay on B would prove nothing")
    load("A")
    cap_ = hip_graph.capture(stream, lambda: chain(e, P, graph, stride, n_table, stream.cuda_stream))
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
        if shape["kernel"] != LAUNCHES:
            failures.append("%d kernel nodes, the headers say %d" % (shape["kernel"], LAUNCHES))
        status = cap_.instantiate()
        if status != 0:
            failures.append("hipGraphInstantiate: %s" % hip_graph.error_name(status))
    if not failures:
        for step, key in enumerate(("A", "B", "A")):
            load(key)
            status = cap_.launch(stream.cuda_stream)
            got = read()
            if status != 0:
                failures.append("replay %d (%s): hipGraphLaunch: %s" % (step + 1, key, hip_graph.error_name(status)))
                break
            failures += differences(got, key, "replay %d on %s" % (step + 1, key))
            if failures:
                break
    torch.cuda.synchronize()
    cap_.destroy()
    load("B")
    chain(e, P, graph, stride, n_table, stream.cuda_stream)
    failures += differences(read(), "B", "a direct call behind the graph")
    e.close()
    counts = "" if shape is None else " kernel=%d memset=%d" % (shape["kernel"], shape["memset"])
    if failures:
        print("keyframe culling chain: FAIL:%s %s" % (counts, " | ".join(failures[:12])), flush=True)
        return 1
    print("keyframe culling chain: PASS%s" % counts, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
