"""The frame's local-map chain on one stream with nothing read back in between, for tests/test_gpu_local_map_chain.py:
  spfe_update_local_map_resident -> spfe_gather_map_points_device (n = point_cap) -> spfe_track_local_map_record_device
  (n = point_cap, on the block's own mp_of_kp_list) -> spfe_local_map_rows_resident
on the panning scene of tests/test_gpu_extents.py (240 x 320, 400 features: the records the extents tests track on; their
64 x 96 handles extract no frame), whose local map is scattered over a map-point table and seen by six
keyframes; and the host-driven route it is compared with: the list of tests/localmap_ref/localmap_ref.c with the exact n_points,
gathered with numpy, uploaded, searched with n = n_points.

    python -m tests.localmap_chain      the chain captured into a hipGraph and replayed on a second input, as
                                        tests/graph_forms.py does it for the *_device forms (one fresh process, one verdict line)
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "localmap_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
sys.path.insert(0, ROOT)
import localmap_ref  # noqa: E402

N_SLOTS, N_BEST, SPARE, POINT_CAP, FILL = 6, 4, 40, 448, 0xA5
OUTPUTS = ("d_block", "d_proj_out", "d_pose_out", "d_rows")
LAUNCHES = 7 + 1 + 5 + 1       # the local map, the gather, TrackLocalMap (tests/graph_forms.py: 5), the rows


def build_world(v, seed):
    """view v of graph_forms.track_scene() -> (case of localmap_cases.KEYS, table dict, spec name -> array / output bytes)"""
    import test_gpu_extents as tge
    rng = np.random.default_rng(seed)
    lm, n_lm = v.lm, v.n_lm
    n_table = n_lm + SPARE
    row_of = rng.permutation(n_table)[:n_lm].astype(np.int32)          # the table row of local-map point i
    table = dict(xyz=np.zeros((n_table, 3), np.float32), normal=np.zeros((n_table, 3), np.float32),
                 dist_range=np.zeros((n_table, 2), np.float32), desc=np.zeros((n_table, 256), np.float32),
                 flags=np.zeros(n_table, np.uint8))
    for k in ("xyz", "normal", "desc", "flags"):
        table[k][row_of] = lm[k]
    table["dist_range"][row_of] = rng.uniform(0.5, 9.0, (n_lm, 2)).astype(np.float32)
    spare = np.setdiff1d(np.arange(n_table), row_of)
    table["flags"][spare[::2]] = 3                                     # searchable rows no keyframe sees: never listed
    entry = tge.association(v.S, v.rc, v.sel_lm, k_from=v.k_last, every=2)    # the holders, as local-map points
    mp_rows = np.where(entry >= 0, row_of[np.maximum(entry, 0)], -1).astype(np.int32)
    rows = np.full((N_SLOTS, tge.KMAX), -1, np.int32)
    first_free = int(entry.max()) + 1                                  # the local-map points behind it are held by nobody
    assert 0 < first_free < n_lm - 8
    for s in range(N_SLOTS):                                           # slots 0-3 are voted; 4 (pushed as a best covisible) and 5 (bad) not
        seen = np.flatnonzero(np.arange(n_lm) % 4 == s) if s < 4 else first_free + rng.permutation(n_lm - first_free)[:(n_lm - first_free) // 2]
        seen = rng.permutation(seen)
        rows[s, :len(seen)] = row_of[seen]
        rows[s, len(seen)] = n_table + 7                               # an entry outside the table
    kf_flags = np.zeros(N_SLOTS, np.uint8)
    kf_flags[5] = 1
    best_cov = np.full((N_SLOTS, N_BEST), -1, np.int32)
    best_cov[0, :2] = [5, 4]
    parent = np.array([-1, 0, 1, 2, 3, 4], np.int32)
    case = dict(kf_mp_of_kp=rows, kf_flags=kf_flags, best_cov=best_cov, parent=parent, mp_flags=table["flags"], mp_of_kp=mp_rows,
                max_keyframes=80, point_cap=POINT_CAP)
    e = v.S.ext
    spec = dict(d_record=v.S.raw[v.rc], d_kf_mp_of_kp=rows, d_kf_flags=kf_flags, d_best_cov=best_cov, d_parent=parent,
                d_t_xyz=table["xyz"], d_t_flags=table["flags"], d_t_normal=table["normal"], d_t_dist_range=table["dist_range"],
                d_t_desc=table["desc"], d_mp_of_kp=mp_rows, d_Tcw=np.ascontiguousarray(v.T_near, np.float32).reshape(-1),
                d_block=e.localmap_out_bytes(N_SLOTS, POINT_CAP, tge.KMAX), d_l_id=4 * POINT_CAP, d_l_xyz=12 * POINT_CAP,
                d_l_normal=12 * POINT_CAP, d_l_dist_range=8 * POINT_CAP, d_l_desc=1024 * POINT_CAP, d_l_flags=POINT_CAP,
                d_proj_out=tge.PROJ_OUT_BYTES, d_pose_out=v.S.dims["pose"], d_rows=4 * tge.KMAX)
    return case, table, spec


def chain(e, P, n_table, stream):
    """the four calls on the addresses P[name], on `stream`: nothing is read back, no tensor is made"""
    import test_gpu_extents as tge
    from sp_orb_slam_amd import extractor as X
    o = X.localmap_offsets(N_SLOTS, POINT_CAP, tge.KMAX)
    e.update_local_map_resident(P["d_kf_mp_of_kp"], tge.KMAX, P["d_kf_flags"], P["d_best_cov"], N_BEST, P["d_parent"], N_SLOTS,
                                P["d_t_flags"], n_table, P["d_mp_of_kp"], tge.KMAX, P["d_block"], POINT_CAP, stream=stream)
    e.gather_map_points_device(P["d_block"] + o["point_idx"], POINT_CAP, P["d_t_xyz"], P["d_t_flags"], P["d_t_normal"],
                               P["d_t_dist_range"], P["d_t_desc"], n_table, P["d_l_id"], P["d_l_xyz"], P["d_l_normal"],
                               P["d_l_dist_range"], P["d_l_desc"], P["d_l_flags"], stream=stream)
    e.track_local_map_record_device(P["d_record"], P["d_l_xyz"], P["d_l_normal"], P["d_l_desc"], P["d_l_flags"], POINT_CAP,
                                    P["d_block"] + o["mp_of_kp_list"], P["d_Tcw"], P["d_proj_out"], P["d_pose_out"], *tge.INTR,
                                    tge.TH_NINLIER_LOW, stream=stream)
    e.local_map_rows_resident(P["d_block"] + o["point_idx"], POINT_CAP, P["d_block"] + o["mp_of_kp_list"], tge.KMAX, P["d_rows"],
                              stream=stream)


def host_route(e, ref, case, table, spec):
    """the reference's list with the exact n, uploaded, through spfe_track_local_map_record_device -> dict(r (the reference's
    result), proj (decoded), pose (bytes), rows (the holders as table rows, converted on the host))"""
    import torch
    import test_gpu_extents as tge
    r = localmap_ref.update(ref, case)
    n = r["n_points"]
    idx = r["point_idx"][:n]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()   # noqa: E731
    d = {k: up(table[k][idx]) for k in ("xyz", "normal", "desc", "flags")}
    d_rec, d_T = up(spec["d_record"]), up(spec["d_Tcw"])
    d_mp = up(r["mp_of_kp_list"])
    d_proj = torch.full((tge.PROJ_OUT_BYTES,), FILL, dtype=torch.uint8, device="cuda")
    d_pose = torch.full((spec["d_pose_out"],), FILL, dtype=torch.uint8, device="cuda")
    e.track_local_map_record_device(d_rec.data_ptr(), d["xyz"].data_ptr(), d["normal"].data_ptr(), d["desc"].data_ptr(),
                                    d["flags"].data_ptr(), n, d_mp.data_ptr(), d_T.data_ptr(), d_proj.data_ptr(), d_pose.data_ptr(),
                                    *tge.INTR, tge.TH_NINLIER_LOW)
    torch.cuda.synchronize()
    mp = d_mp.cpu().numpy().view(np.int32)
    rows = np.where((mp >= 0) & (mp < n), idx[np.clip(mp, 0, max(n - 1, 0))] if n else -1, -1).astype(np.int32)
    return dict(r=r, proj=e.decode_proj_out(d_proj.cpu().numpy(), n), pose=d_pose.cpu().numpy(), rows=rows, mp_list=mp)


def compare(e, got, want, kmax):
    """the outputs of the device chain against the host route -> list of findings"""
    from sp_orb_slam_amd import extractor as X
    found = []
    r, n = want["r"], want["r"]["n_points"]
    o = X.localmap_offsets(N_SLOTS, POINT_CAP, kmax)
    block = got["d_block"].copy()
    lst = block[o["mp_of_kp_list"]:o["mp_of_kp_list"] + 4 * kmax].view(np.int32).copy()
    block[o["mp_of_kp_list"]:o["mp_of_kp_list"] + 4 * kmax] = r["block"][o["mp_of_kp_list"]:o["mp_of_kp_list"] + 4 * kmax]
    if block.tobytes() != r["block"].tobytes():
        found.append("the local-map block differs from localmap_ref.c outside mp_of_kp_list")
    if not np.array_equal(lst, want["mp_list"]):
        found.append("the holders as list positions behind TrackLocalMap differ in %d keypoints" % (lst != want["mp_list"]).sum())
    if got["d_pose_out"].tobytes() != want["pose"].tobytes():
        found.append("the pose block differs in %d bytes" % (got["d_pose_out"] != want["pose"]).sum())
    if not np.array_equal(got["d_rows"].view(np.int32), want["rows"]):
        found.append("the holders as table rows differ")
    g = e.decode_proj_out(got["d_proj_out"], n)
    for k in ("n_matches", "n_to_match"):
        if g[k] != want["proj"][k]:
            found.append("%s %d, the host route %d" % (k, g[k], want["proj"][k]))
    for k in ("kp_of_mp", "proj_uv", "view_cos", "in_view"):
        if g[k].tobytes() != want["proj"][k].tobytes():
            found.append("search output %s of the first n_points points differs" % k)
    full = e.decode_proj_out(got["d_proj_out"], POINT_CAP)
    if (full["kp_of_mp"][n:] != -1).any() or full["in_view"][n:].any():
        found.append("a padding row of the list was matched or in view")
    return found


def main():
    """A and B: the two views of the scene.  Direct calls (the first sizes every scratch: it is the only size), the host route of
    each, one capture, three replays A, B, A, a direct call behind the graph."""
    import torch
    import graph_forms as gf
    import hip_graph
    import test_gpu_extents as tge
    S, V = gf.track_scene()
    e = S.ext
    ref = localmap_ref.build(tempfile.mkdtemp(prefix="localmap_chain_"))
    worlds = {key: build_world(v, seed) for key, v, seed in (("A", V[0], 11), ("B", V[1], 12))}
    names = list(worlds["A"][2])
    size = {k: (int(v) if gf.is_out(v) else len(gf.raw_bytes(v))) for k, v in worlds["A"][2].items()}
    assert all(size[k] == (int(v) if gf.is_out(v) else len(gf.raw_bytes(v))) for k, v in worlds["B"][2].items())
    n_table = len(worlds["A"][1]["flags"])
    assert n_table == len(worlds["B"][1]["flags"])
    bufs = {k: torch.full((size[k] + 16,), FILL, dtype=torch.uint8, device="cuda") for k in names}
    P = {k: t.data_ptr() for k, t in bufs.items()}
    img = {key: {k: torch.from_numpy(gf.raw_bytes(w[2][k]).copy()) for k in names if not gf.is_out(w[2][k])} for key, w in worlds.items()}
    stream = torch.cuda.Stream()

    def load(key):
        for k in names:
            if k in img[key]:
                bufs[k][:size[k]].copy_(img[key][k])
            else:
                bufs[k].fill_(FILL)
        torch.cuda.synchronize()

    def read():
        torch.cuda.synchronize()
        return {k: bufs[k][:size[k]].cpu().numpy() for k in OUTPUTS}

    failures, want = [], {}
    for key in ("A", "B"):
        load(key)
        chain(e, P, n_table, stream.cuda_stream)
        want[key] = read()
        case, table, spec = worlds[key]
        host = host_route(e, ref, case, table, spec)
        failures += ["direct chain on %s: %s" % (key, f) for f in compare(e, want[key], host, tge.KMAX)]
        g = e.decode_pose_out(want[key]["d_pose_out"], tge.KMAX)
        print("%s: n_points %d of cap %d, local keyframes %s, matches %d, inliers %d, verdict %d" % (
            key, host["r"]["n_points"], POINT_CAP, host["r"]["local_kf"].tolist(), g["n_matches"], g["n_inliers"], g["verdict"]))
        if not (host["r"]["n_points"] < POINT_CAP and g["n_matches"] > 20 and host["r"]["n_local_kf"] > host["r"]["n_voted"] >= 4):
            failures.append("%s: the case does not exercise the chain" % key)
    if any(np.array_equal(want["A"][k], want["B"][k]) for k in OUTPUTS):
        failures.append("A and B give the same output: the replay on B would prove nothing")
    load("A")
    cap = hip_graph.capture(stream, lambda: chain(e, P, n_table, stream.cuda_stream))
    shape = None
    if not cap.ok:
        failures.append("capture refused or invalidated: %s" % cap.why())
    else:
        shape = cap.shape()
        print("graph", shape)
        if shape["other"] or shape["memset"]:
            failures.append("nodes other than kernels: %s, %d memsets" % (shape["other"], shape["memset"]))
        if shape["roots"] != 1 or shape["edges"] != shape["nodes"] - 1:
            failures.append("not one chain: %d nodes, %d edges, %d roots" % (shape["nodes"], shape["edges"], shape["roots"]))
        if shape["kernel"] != LAUNCHES:
            failures.append("%d kernel nodes, the headers say %d" % (shape["kernel"], LAUNCHES))
        status = cap.instantiate()
        if status != 0:
            failures.append("hipGraphInstantiate: %s" % hip_graph.error_name(status))
        else:
            for step, key in enumerate(("A", "B", "A")):
                load(key)
                status = cap.launch(stream.cuda_stream)
                got = read()
                if status != 0:
                    failures.append("replay %d (%s): hipGraphLaunch: %s" % (step + 1, key, hip_graph.error_name(status)))
                    break
                for k in OUTPUTS:
                    dd = np.flatnonzero(got[k] != want[key][k])
                    if len(dd):
                        failures.append("replay %d on %s: %r differs from the direct call in %d byte(s), the first at %d" % (
                            step + 1, key, k, len(dd), dd[0]))
    torch.cuda.synchronize()
    cap.destroy()
    load("B")
    chain(e, P, n_table, stream.cuda_stream)
    again = read()
    failures += ["a direct call behind the graph: %r differs" % k for k in OUTPUTS if not np.array_equal(again[k], want["B"][k])]
    e.close()
    counts = "" if shape is None else " kernel=%d memset=%d" % (shape["kernel"], shape["memset"])
    if failures:
        print("local-map chain: FAIL:%s %s" % (counts, " | ".join(failures)), flush=True)
        return 1
    print("local-map chain: PASS%s" % counts, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
