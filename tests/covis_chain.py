"""A keyframe insertion as ONE captured graph, from the keyframe rows to the loop candidates and the local map, for
tests/test_gpu_covisibility_chain.py.  Four calls on one stream, nothing read back in between:
  spfe_covis_reset_slots_resident (the new slot) -> spfe_update_connections_resident (both tables) ->
  spfe_detect_loop_candidates_device (its 10-column table, d_connected and d_covisible straight from the graph state: rows cur_slot
  of d_conn_slot and d_ord_slot, count min(conn_cap, n_slots)) -> spfe_update_local_map_resident (the 20-column table and d_parent
  from the graph state)
against the three host references chained in Python (tests/covis_ref, tests/loopdet_ref, tests/localmap_ref).

    python -m tests.covis_chain      two graphs (keyframe K, then keyframe K + 1 on the state the first left) captured once and
                                     replayed on two inputs, as tests/localmap_chain.py does it (one fresh process, one verdict
                                     line).  The process's hardware queue count is left as the machine sets it.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "covis_ref", "loopdet_ref", "localmap_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
sys.path.insert(0, ROOT)
import covis_cases as cc  # noqa: E402
import covis_ref  # noqa: E402
import localmap_ref  # noqa: E402
import loopdet_cases  # noqa: E402
import loopdet_ref  # noqa: E402

N_SLOTS, K_NEW, STRIDE, N_TABLE, CONN_CAP, TH, DIM, POINT_CAP, FILL = 48, 30, 40, 400, 48, 3, 64, 512, 0xA5
N_BEST_A, N_BEST_B = 20, 10
N_CONN = min(CONN_CAP, N_SLOTS)
BLOCKS = ("d_covis_out", "d_loop_out", "d_lm_out")
LAUNCHES = 1 + 5 + 3 + 7       # the reset, UpdateConnections, the loop detection, the local map
PRM = ("min_score_init", "min_score_floor", "retain_ratio")
HOST_ONLY = ("prm", "row_next")


def build_world(ref, seed):
    """the map as K_NEW keyframes left it (state and tables by covis_ref.c, the tables -1 where nobody wrote), the row of the new
    keyframe at K_NEW and the one to follow as row_next -> dict name -> array: the images of every device buffer but the blocks"""
    rows, kf_flags, mp_flags = cc.generated_rows(seed, N_SLOTS, STRIDE, N_TABLE, window=3 * STRIDE, p_bad_kf=0.08)
    row_next = rows[K_NEW + 1].copy()                                      # the host appends it in front of the second insertion
    rows[K_NEW + 1:] = -1
    kf_flags[K_NEW:] = 0
    state = covis_ref.new_state(N_SLOTS, CONN_CAP, fill=0x5A)            # the slots not yet inserted hold rubbish: the reset's work
    covis_ref.reset(ref, state, 0, K_NEW)
    ta, tb = np.full((N_SLOTS, N_BEST_A), -1, np.int32), np.full((N_SLOTS, N_BEST_B), -1, np.int32)
    seen = rows.copy()
    seen[K_NEW:] = -1
    for s in range(K_NEW):
        covis_ref.update(ref, seen, kf_flags, mp_flags, state, s, TH, 0, ta, tb)
    lc = loopdet_cases.generated(seed, N_SLOTS, DIM, cur=K_NEW).arrays()
    in_db = np.ascontiguousarray(lc["in_db"], np.uint8).copy()
    in_db[K_NEW:] = 0
    w = dict(d_kf_mp_of_kp=rows, d_kf_flags=kf_flags, d_mp_flags=mp_flags, d_gdesc=np.ascontiguousarray(lc["gdesc"], np.float32),
             d_in_db=in_db, d_best_a=ta, d_best_b=tb, row_next=row_next)
    w.update({"d_" + k: state[k] for k in covis_ref.STATE})
    w["prm"] = [float(lc[k]) for k in PRM]
    return w


def chain(e, P, graph, cur, prm, stream):
    """the four calls on the addresses P[name], on `stream`: nothing is read back, no tensor is made"""
    e.covis_reset_slots_resident(graph, cur, 1, stream=stream)
    e.update_connections_resident(graph, P["d_kf_mp_of_kp"], STRIDE, P["d_kf_flags"], P["d_mp_flags"], N_TABLE, cur, P["d_covis_out"],
                                  th=TH, origin_slot=0, d_best_cov_a=P["d_best_a"], n_best_a=N_BEST_A, d_best_cov_b=P["d_best_b"],
                                  n_best_b=N_BEST_B, stream=stream)
    e.detect_loop_candidates_device(P["d_gdesc"], DIM, P["d_kf_flags"], P["d_in_db"], P["d_best_b"], N_SLOTS, cur,
                                    P["d_conn_slot"] + 4 * cur * CONN_CAP, N_CONN, P["d_ord_slot"] + 4 * cur * CONN_CAP, N_CONN,
                                    P["d_loop_out"], *prm, stream=stream)
    e.update_local_map_resident(P["d_kf_mp_of_kp"], STRIDE, P["d_kf_flags"], P["d_best_a"], N_BEST_A, P["d_parent"], N_SLOTS,
                                P["d_mp_flags"], N_TABLE, P["d_kf_mp_of_kp"] + 4 * cur * STRIDE, STRIDE, P["d_lm_out"], POINT_CAP,
                                stream=stream)


def host_route(refs, w, state, ta, tb, cur):
    """the same four steps through the three host references, on the host copies (updated in place) -> the three blocks"""
    rc, rl, rm = refs
    rows, kf_flags, mp_flags = w["d_kf_mp_of_kp"], w["d_kf_flags"], w["d_mp_flags"]
    covis_ref.reset(rc, state, cur, 1)
    c = covis_ref.update(rc, rows, kf_flags, mp_flags, state, cur, TH, 0, ta, tb)
    case = dict(gdesc=w["d_gdesc"], kf_flags=kf_flags, in_db=w["d_in_db"], best_cov=tb, cur_slot=cur,
                connected=state["conn_slot"][cur, :N_CONN], covisible=state["ord_slot"][cur, :N_CONN], **dict(zip(PRM, w["prm"])))
    d = loopdet_ref.detect(rl, case)
    m = localmap_ref.update(rm, dict(kf_mp_of_kp=rows, kf_flags=kf_flags, best_cov=ta, parent=state["parent"], mp_flags=mp_flags,
                                     mp_of_kp=rows[cur], max_keyframes=80, point_cap=POINT_CAP))
    return dict(d_covis_out=c["block"], d_loop_out=d["block"], d_lm_out=m["block"], covis=c, loop=d, lm=m)


def main():
    import torch
    import hip_graph
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    e = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    tmp = tempfile.mkdtemp(prefix="covis_chain_")
    refs = (covis_ref.build(tmp), loopdet_ref.build(tmp), localmap_ref.build(tmp))
    worlds = {"A": build_world(refs[0], 701), "B": build_world(refs[0], 702)}
    prm = worlds["A"]["prm"]
    assert prm == worlds["B"]["prm"]
    raw = lambda a: np.ascontiguousarray(a).reshape(-1).view(np.uint8)   # noqa: E731
    size = {k: len(raw(v)) for k, v in worlds["A"].items() if k not in HOST_ONLY}
    size.update(d_covis_out=e.covis_out_bytes(N_SLOTS, CONN_CAP), d_loop_out=e.loopdet_out_bytes(N_SLOTS),
                d_lm_out=e.localmap_out_bytes(N_SLOTS, POINT_CAP, STRIDE))
    bufs = {k: torch.full((n + 16,), FILL, dtype=torch.uint8, device="cuda") for k, n in size.items()}
    P = {k: t.data_ptr() for k, t in bufs.items()}
    graph = X.covis_graph({k: P["d_" + k] for k in covis_ref.STATE}, N_SLOTS, CONN_CAP)
    img = {key: {k: torch.from_numpy(raw(v).copy()) for k, v in w.items() if k not in HOST_ONLY} for key, w in worlds.items()}
    stream = torch.cuda.Stream()
    written = ["d_" + k for k in covis_ref.STATE] + ["d_best_a", "d_best_b"] + list(BLOCKS)

    def load(key):
        for k in size:
            if k in img[key]:
                bufs[k][:size[k]].copy_(img[key][k])
            else:
                bufs[k].fill_(FILL)
        torch.cuda.synchronize()

    def append_next_row(key):
        """the row of keyframe K_NEW + 1 into the resident rows, as the host does in front of its insertion"""
        torch.cuda.synchronize()
        at = 4 * (K_NEW + 1) * STRIDE
        bufs["d_kf_mp_of_kp"][at:at + 4 * STRIDE].copy_(torch.from_numpy(raw(worlds[key]["row_next"]).copy()))
        torch.cuda.synchronize()

    def read():
        torch.cuda.synchronize()
        return {k: bufs[k][:size[k]].cpu().numpy() for k in written}

    def expected(key):
        """the host route for K_NEW, then K_NEW + 1 on what it left -> per keyframe the bytes of every written buffer"""
        w = dict(worlds[key], d_kf_mp_of_kp=worlds[key]["d_kf_mp_of_kp"].copy())
        state = {k: w["d_" + k].copy() for k in covis_ref.STATE}
        ta, tb = w["d_best_a"].copy(), w["d_best_b"].copy()
        out = []
        for cur in (K_NEW, K_NEW + 1):
            if cur == K_NEW + 1:
                w["d_kf_mp_of_kp"][cur] = w["row_next"]
            h = host_route(refs, w, state, ta, tb, cur)
            want = {"d_" + k: raw(state[k]).copy() for k in covis_ref.STATE}
            want.update(d_best_a=raw(ta).copy(), d_best_b=raw(tb).copy(), loop_mask=loopdet_ref.written_mask(h["loop"], N_SLOTS),
                        **{k: h[k] for k in BLOCKS})
            out.append((want, h))
        return out

    def differences(got, want, what):
        """every written buffer against the host route; of the loop detection's block the bytes that call writes (the lists' tails
        keep what the buffer held: the call before)"""
        found = []
        for k in written:
            bad = got[k] != want[k]
            if k == "d_loop_out":
                bad &= want["loop_mask"]
            if bad.any():
                found.append("%s: %r differs from the host references in %d byte(s), the first at %d" % (
                    what, k, bad.sum(), np.flatnonzero(bad)[0]))
        return found

    failures, want = [], {key: expected(key) for key in worlds}
    for key in ("A", "B"):                # direct calls first: they size the handle's scratch, the only size there is
        load(key)
        for i, cur in enumerate((K_NEW, K_NEW + 1)):
            if i:
                append_next_row(key)
            chain(e, P, graph, cur, prm, stream.cuda_stream)
            failures += differences(read(), want[key][i][0], "direct chain on %s, keyframe %d" % (key, cur))
            h = want[key][i][1]
            print("%s keyframe %d: linked %d of %d sharers, parent %d, loop candidates %d of %d passed, local keyframes %d, points %d" % (
                key, cur, h["covis"]["n_linked"], h["covis"]["n_counter"], h["covis"]["parent_set"], h["loop"]["n_cand"],
                h["loop"]["n_pass"], h["lm"]["n_local_kf"], h["lm"]["n_points"]))
            if not (h["covis"]["status"] == 0 and 2 <= h["covis"]["n_linked"] < h["covis"]["n_counter"] and h["covis"]["parent_set"] >= 0
                    and h["loop"]["status"] == loopdet_ref.BAD_LIST_INDEX      # the -1 padding of the two lists, skipped
                    and h["loop"]["n_pass"] >= 1 - i and h["loop"]["n_scored"] > h["covis"]["n_linked"]
                    and h["lm"]["n_local_kf"] > h["covis"]["n_linked"] and h["lm"]["n_points"] > STRIDE // 2):
                failures.append("%s keyframe %d: the case does not exercise the chain" % (key, cur))
    if any(want["A"][0][0][k].tobytes() == want["B"][0][0][k].tobytes() for k in BLOCKS):
        failures.append("A and B give the same block: the replay on B would prove nothing")
    load("A")
    caps, shapes = [], []
    for cur in (K_NEW, K_NEW + 1):
        cap = hip_graph.capture(stream, lambda: chain(e, P, graph, cur, prm, stream.cuda_stream))
        caps.append(cap)
        if not cap.ok:
            failures.append("capture for keyframe %d refused or invalidated: %s" % (cur, cap.why()))
            continue
        shape = cap.shape()
        shapes.append(shape)
        print("graph", cur, shape)
        if shape["other"] or shape["memset"]:
            failures.append("nodes other than kernels: %s, %d memsets" % (shape["other"], shape["memset"]))
        if shape["roots"] != 1 or shape["edges"] != shape["nodes"] - 1:
            failures.append("not one chain: %d nodes, %d edges, %d roots" % (shape["nodes"], shape["edges"], shape["roots"]))
        if shape["kernel"] != LAUNCHES:
            failures.append("%d kernel nodes, the headers say %d" % (shape["kernel"], LAUNCHES))
        status = cap.instantiate()
        if status != 0:
            failures.append("hipGraphInstantiate: %s" % hip_graph.error_name(status))
    if not failures:
        for step, key in enumerate(("A", "B", "A")):
            load(key)
            for i, cap in enumerate(caps):       # keyframe K_NEW, then K_NEW + 1 on the state the first replay left on the device
                if i:
                    append_next_row(key)
                status = cap.launch(stream.cuda_stream)
                got = read()
                if status != 0:
                    failures.append("replay %d (%s): hipGraphLaunch: %s" % (step + 1, key, hip_graph.error_name(status)))
                    break
                failures += differences(got, want[key][i][0], "replay %d on %s, keyframe %d" % (step + 1, key, K_NEW + i))
            if failures:
                break
    torch.cuda.synchronize()
    for cap in caps:
        cap.destroy()
    load("B")
    chain(e, P, graph, K_NEW, prm, stream.cuda_stream)
    failures += differences(read(), want["B"][0][0], "a direct call behind the graphs")
    e.close()
    counts = "" if len(shapes) != 2 else " kernel=%d+%d memset=%d" % (shapes[0]["kernel"], shapes[1]["kernel"],
                                                                      shapes[0]["memset"] + shapes[1]["memset"])
    if failures:
        print("covisibility chain: FAIL:%s %s" % (counts, " | ".join(failures[:12])), flush=True)
        return 1
    print("covisibility chain: PASS%s" % counts, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
