"""What the GPU tests of the gather in front of the local bundle adjustment and of the application behind it share: the buffers of a
case (lba_cases) at exactly their documented sizes, one call through each form of the library on given addresses, and the comparison
of the block and of everything the call may edit with lba_ref.c byte for byte.  torch is imported inside the functions."""
import numpy as np

import lba_cases as lc
import lba_ref as lr

from sp_orb_slam_amd import extractor as X

FILL = lr.FILL
GUARD = 1024          # bytes behind the block that must keep the preset
APPLY_EDITS = ("rows", "mp_flags", "nobs", "ref_slot", "xyz", "Tcw")


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def buffers(c):
    """name -> the array a pointer argument of the case's resident form points at (its initial contents), or the bytes of an output;
    every one at exactly the extent include/spfe.h documents.  The gather's d_ord_slot is the whole [n_slots][conn_cap] array: row
    cur_slot holds the case's ord_row, every other row poison that must not be read as a slot."""
    if c["op"] == "gather":
        n = c["rows"].shape[0]
        ord_slot = np.full((n, len(c["ord_row"])), 0x5A5A5A5A, np.int32)
        ord_slot[int(c["cur_slot"])] = c["ord_row"]
        b = {k: c[k] for k in ("rows", "kf_flags", "mp_flags", "xyz", "Tcw")}
        b.update(ord_slot=ord_slot, d_out=lr.gather_offsets(c["kf_cap"], c["point_cap"], c["edge_cap"])["out_bytes"])
    else:
        b = {k: c[k] for k in lr.WORLD}
        b.update(gather=c["gather"], ba=c["ba"], d_out=lr.apply_offsets(c["point_cap"], c["edge_cap"], c["bad_cap"])["out_bytes"])
    return b


def extents(c):
    """name -> bytes, by the comments above the declarations in include/spfe.h"""
    n, stride = c["rows"].shape
    nt = len(c["mp_flags"])
    e = dict(rows=4 * stride * n, kf_flags=n, mp_flags=nt, xyz=12 * nt, Tcw=64 * n)
    if c["op"] == "gather":
        e.update(ord_slot=4 * len(c["ord_row"]) * n, d_out=X.lba_gather_offsets(c["kf_cap"], c["point_cap"], c["edge_cap"])["out_bytes"])
    else:
        g = np.ascontiguousarray(c["gather"][:64]).view(np.int32)
        n_kf, npts, E = int(g[4]), int(g[5]), int(g[8])
        sane = 1 <= n_kf <= c["kf_cap"] and 0 <= npts <= c["point_cap"] and 0 <= E <= c["edge_cap"]
        e.update(nobs=4 * nt, ref_slot=4 * nt, gather=X.lba_gather_offsets(c["kf_cap"], c["point_cap"], c["edge_cap"])["out_bytes"],
                 ba=lr.ba_offsets(n_kf, npts, E)["out_bytes"] if sane else len(c["ba"]),
                 d_out=X.lba_apply_offsets(c["point_cap"], c["edge_cap"], c["bad_cap"])["out_bytes"])
    return e


def outputs(c):
    """the buffers the case's call may write"""
    return ("d_out",) if c["op"] == "gather" else APPLY_EDITS + ("d_out",)


def call(ext, P, c, stream=None):
    """the case's resident form on the addresses P[name]: nothing is read back, no tensor is made"""
    n, stride = c["rows"].shape
    nt = len(c["mp_flags"])
    if c["op"] == "gather":
        ext.gather_local_ba_resident(P["ord_slot"], len(c["ord_row"]), P["rows"], stride, P["kf_flags"], n, P["mp_flags"], P["xyz"], nt, P["Tcw"],
                                     int(c["cur_slot"]), P["d_out"], origin_slot=int(c["origin_slot"]), kf_cap=int(c["kf_cap"]),
                                     free_cap=int(c["free_cap"]), point_cap=int(c["point_cap"]), edge_cap=int(c["edge_cap"]), stream=stream)
    else:
        ext.apply_local_ba_resident(P["gather"], P["ba"], P["rows"], stride, P["kf_flags"], n, P["mp_flags"], P["nobs"], P["ref_slot"], P["xyz"],
                                    nt, P["Tcw"], int(c["kf_cap"]), int(c["point_cap"]), int(c["edge_cap"]), P["d_out"], bad_cap=int(c["bad_cap"]),
                                    stream=stream)


def want_of(ref, c):
    """the reference's bytes of every output buffer of the case"""
    w, r = lc.run_ref(ref, c)
    want = {k: raw(w[k]) for k in outputs(c) if k != "d_out"}
    want["d_out"] = r["block"]
    return want, r


def run_resident(ext, c, shift=0, stream=None):
    """the resident form on fresh device buffers (the rows `shift` bytes off a 256-byte boundary), the block and a guard behind it
    filled with FILL -> name -> bytes of every output and of every input (which must come back unchanged); the guard is checked"""
    import torch
    tens, P = {}, {}
    spec = buffers(c)
    for k, v in spec.items():
        if isinstance(v, (int, np.integer)):
            t = torch.full((int(v) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        else:
            off = shift if k == "rows" else 0
            t = torch.zeros(off + max(raw(v).size, 16), dtype=torch.uint8, device="cuda")
            t[off:off + raw(v).size] = torch.from_numpy(raw(v).copy()).cuda()
            t = t[off:]
        tens[k], P[k] = t, t.data_ptr()
    call(ext, P, c, stream)
    torch.cuda.synchronize()
    got = {}
    for k, v in spec.items():
        nb = int(v) if isinstance(v, (int, np.integer)) else raw(v).size
        host = tens[k].cpu().numpy()
        got[k] = host[:nb].copy()
        if k == "d_out":
            assert (host[nb:] == FILL).all(), "bytes behind the block were written"
        elif k not in outputs(c):
            assert got[k].tobytes() == raw(v).tobytes(), "the read-only input %r was written" % k
    return got


def run_host(ext, c):
    """the host-array form on a copy -> name -> bytes of every output"""
    w = lr.copy_world(c)
    if c["op"] == "gather":
        block = ext.gather_local_ba(c["ord_row"], w["rows"], w["kf_flags"], w["mp_flags"], w["xyz"], w["Tcw"], int(c["cur_slot"]),
                                    origin_slot=int(c["origin_slot"]), kf_cap=int(c["kf_cap"]), free_cap=int(c["free_cap"]),
                                    point_cap=int(c["point_cap"]), edge_cap=int(c["edge_cap"]), fill=FILL)
        assert not lr.diff_world(w, c)
    else:
        block = ext.apply_local_ba(c["gather"], c["ba"], w["rows"], w["kf_flags"], w["mp_flags"], w["nobs"], w["ref_slot"], w["xyz"], w["Tcw"],
                                   int(c["kf_cap"]), int(c["point_cap"]), int(c["edge_cap"]), bad_cap=int(c["bad_cap"]), fill=FILL)
        assert w["kf_flags"].tobytes() == c["kf_flags"].tobytes()
    got = {k: raw(w[k]) for k in outputs(c) if k != "d_out"}
    got["d_out"] = block
    return got


def same(got, want, c, what):
    for k in outputs(c):
        g, r = np.asarray(got[k]), np.asarray(want[k])
        assert len(g) == len(r), (what, k, len(g), len(r))
        if g.tobytes() != r.tobytes():
            if k == "d_out":
                if c["op"] == "gather":
                    a = (int(c["kf_cap"]), int(c["point_cap"]), int(c["edge_cap"]))
                    dg, dr, fields = lr.decode_gather(g, *a), lr.decode_gather(r, *a), lr.GATHER_FIELDS
                    arrays = ("kf_slot", "fixed", "point_idx", "obs_start", "obs", "edges", "Tcw", "xyz")
                else:
                    a = (int(c["point_cap"]), int(c["edge_cap"]), int(c["bad_cap"]))
                    dg, dr, fields = lr.decode_apply(g, *a), lr.decode_apply(r, *a), lr.APPLY_FIELDS
                    arrays = ("bad_point", "obs_start", "obs", "ref_slot")
                for f in fields:
                    assert dg[f] == dr[f], (what, f, dg[f], dr[f])
                for f in arrays:
                    x, y = dg[f].reshape(-1), dr[f].reshape(-1)
                    bad = np.flatnonzero(x.view(np.uint8) != y.view(np.uint8)) // x.itemsize
                    assert not len(bad), (what, f, bad[:8].tolist(), x[bad[:8]].tolist(), y[bad[:8]].tolist())
            bad = np.flatnonzero(g != r)[:8]
            assert False, (what, k, bad.tolist(), g[bad].tolist(), r[bad].tolist())


def check(ext, ref, c, shift=0, host=True, what=""):
    """one call through lba_ref.c, the resident form and (host) the host-array form, all from copies of the case's world -> the
    reference's result"""
    want, r = want_of(ref, c)
    same(run_resident(ext, c, shift), want, c, what + ", resident form")
    if host:
        same(run_host(ext, c), want, c, what + ", host form")
    return r


# ---- the chain on records of a handle: the scene of tests/test_gpu_local_ba.py as resident arrays ------------------------------------
CHAIN = dict(n_slots=8, conn_cap=4, kf_cap=8, free_cap=4, point_cap=256, edge_cap=2048, bad_cap=16)


def records_world(S, variant=0):
    """the six records of the scene S as a resident map: slot f holds frame f, slots 6 and 7 hold no keyframe; four points with
    three or more observations swap their keypoints of slot 3 with another, two pairs at least 15 pixels apart: four gross outliers
    (variant: which pairs, and a small shift of every position) -> (world, ord_slot int32 [n_slots][conn_cap], the gather's parameters)"""
    n_frames, n = len(S.Tcw), len(S.xyz)
    kmax = S.ext.layout.kmax
    w = lr.new_world(CHAIN["n_slots"], kmax, n + 5)
    w["kf_flags"][n_frames:] = 1
    for p, f, kp in S.edges.tolist():
        w["rows"][f, kp] = p
    w["xyz"][:n] = S.xyz + np.float32(variant) / 512
    w["Tcw"][:n_frames] = S.Tcw
    per_point = np.bincount(S.edges[:, 0], minlength=n)
    in3 = {int(p): int(kp) for p, f, kp in S.edges.tolist() if f == 3 and per_point[p] >= 3}
    xy, cand, pairs, used = S.recs[3].kp_xy, sorted(in3), [], set()
    for i, p in enumerate(cand):
        for q in cand[i + 1:]:
            if p not in used and q not in used and np.abs(xy[in3[p]] - xy[in3[q]]).max() >= 15:
                pairs.append((p, q))
                used |= {p, q}
    take = pairs[2 * variant:2 * variant + 2]
    assert len(take) == 2, (len(cand), len(pairs))
    for p, q in take:
        w["rows"][3, in3[p]], w["rows"][3, in3[q]] = q, p
    lc.settle(w)
    ord_slot = np.full((CHAIN["n_slots"], CHAIN["conn_cap"]), -1, np.int32)
    ord_slot[0, :3] = [1, 2, 3]
    prm = dict(cur_slot=0, origin_slot=-1, **{k: CHAIN[k] for k in ("kf_cap", "free_cap", "point_cap", "edge_cap")})
    return w, ord_slot, prm


def reference_chain(S, ref, mref, w, ord_slot, prm, intr):
    """lba_ref.c's gather, ba_ref.c on its problem (observations and information from the records, as the record form reads them),
    lba_ref.c's application and mp_ref.c's normal-and-depth refresh, in sequence on a copy of the world
    -> dict(g, ba, a, mp: the four results; world: the arrays behind the chain)"""
    import ba_ref
    import mp_ref
    n_slots, kmax = w["rows"].shape
    hw = lr.copy_world(w)
    g = lr.gather(ref, hw, ord_slot[prm["cur_slot"]], prm)
    n_kf, m, E = g["n_kf"], g["n_points"], g["n_edges"]
    assert g["status"] == 0 and g["kf_slot"][:4].tolist() == [0, 1, 2, 3] and sorted(g["kf_slot"][4:n_kf].tolist()) == [4, 5] and m == len(S.xyz)
    assert g["fixed"][:n_kf].tolist() == [0, 0, 0, 0, 1, 1]
    edges = g["edges"][:E]
    c = dict(edges=edges, obs_xy=np.stack([S.recs[g["kf_slot"][b]].kp_xy[kp] for _, b, kp in edges.tolist()]).astype(np.float32),
             inv_sigma2=np.stack([S.recs[g["kf_slot"][b]].cov2_inv[kp] for _, b, kp in edges.tolist()]).astype(np.float32),
             Tcw=g["Tcw"][:n_kf], fixed=g["fixed"][:n_kf], xyz=g["xyz"][:m], intr=np.array(intr, np.float32), schedule=np.int32(0),
             iterations=np.array([5, 10], np.int32), robust=np.int32(1), inv_sigma2_full=np.float32(1), stop_reads=np.int32(-1))
    ba = ba_ref.solve(S.ref, c, fill=0x5A)
    a = lr.apply(ref, hw, g["block"], ba["block"], dict(prm, bad_cap=CHAIN["bad_cap"]))
    kf_desc = np.zeros((n_slots, kmax, 256), np.float32)
    for f, r in enumerate(S.recs):
        kf_desc[f, :r.K] = r.descriptors[:r.K]
    mc = dict(kf_flags=hw["kf_flags"], kf_K=np.array([r.K for r in S.recs] + [-1] * (n_slots - len(S.recs)), np.int32),
              kf_status=np.zeros(n_slots, np.int32), Tcw=hw["Tcw"], kf_desc=kf_desc, point_idx=g["point_idx"][:m], obs_start=a["obs_start"][:m + 1],
              obs=a["obs"][:g["n_obs"]], ref_slot=a["ref_slot"][:m], xyz=hw["xyz"], flags=hw["mp_flags"], mode=X.MP_NORMAL_DEPTH, level_scale=1.0,
              top_scale=1.0)
    return dict(g=g, ba=ba, a=a, mp=mp_ref.refresh(mref, mc), world=hw)


def apply_and_refresh(e, P, d_g, d_ba, d_a, d_mp, m, n_obs, n_table, stride, stream):
    """the two calls behind the solver on the addresses given: the application, then UpdateNormalAndDepth of the listed points with
    d_point_idx inside the gather's block and the lists inside the application's"""
    go = X.lba_gather_offsets(CHAIN["kf_cap"], CHAIN["point_cap"], CHAIN["edge_cap"])
    ao = X.lba_apply_offsets(CHAIN["point_cap"], CHAIN["edge_cap"], CHAIN["bad_cap"])
    n_slots = CHAIN["n_slots"]
    e.apply_local_ba_resident(d_g, d_ba, P["rows"], stride, P["kf_flags"], n_slots, P["mp_flags"], P["nobs"], P["ref_slot"], P["xyz"], n_table,
                              P["Tcw"], CHAIN["kf_cap"], CHAIN["point_cap"], CHAIN["edge_cap"], d_a, bad_cap=CHAIN["bad_cap"], stream=stream)
    e.refresh_map_points_device(P["kf_records"], P["kf_flags"], P["Tcw"], n_slots, d_g + go["point_idx"], d_a + ao["obs_start"], d_a + ao["obs"],
                                d_a + ao["ref_slot"], m, n_obs, P["xyz"], P["mp_flags"], P["normal"], P["dist_range"], P["desc"], n_table, d_mp,
                                mode=X.MP_NORMAL_DEPTH, stream=stream)
