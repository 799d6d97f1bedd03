"""What the GPU tests of map-point culling share: the buffers of a case (mpcull_cases) at exactly their documented sizes, one call
through each form of the library on given addresses, and the comparison of the block and of everything the call may edit with
mpcull_ref.c byte for byte.  torch is imported inside the functions."""
import numpy as np

import mpcull_cases as mc
import mpcull_ref as mr

from sp_orb_slam_amd import extractor as X

FILL = mr.FILL
GUARD = 1024          # bytes behind the block that must keep the preset
STAT_STATE = ("flags", "found", "visible")     # the arrays spfe_track_statistics_resident touches: the others are passed as null


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def buffers(c):
    """name -> the array a pointer argument of the case's resident form points at (its initial contents), or the bytes of an output;
    every one at exactly the extent include/spfe.h documents"""
    op = c["op"]
    if op == "cull":
        b = {k: c[k] for k in ("rows", "kf_flags") + mr.STATE}
        b["d_out"] = mr.offsets(len(c["recent"]), int(c["bad_cap"]))["out_bytes"]
    elif op == "admit":
        b = {k: c[k] for k in ("rows", "xyz") + mr.STATE}
        b["tri"] = c["tri"]
        b["neigh_slot"] = np.asarray(c["neigh_slot"], np.int32)
        b["d_out"] = mr.ADMIT_OUT_BYTES
    else:
        b = {k: c[k] for k in STAT_STATE}
        n_kp, cap = len(c["entry"]), len(c["point_idx"])
        if n_kp:
            b["entry"], b["after"] = c["entry"], c["after"]
        b["point_idx"] = c["point_idx"]
        proj = np.full(X.PROJ_OFF_VIEW + cap, 0x5A, np.uint8)       # the search's block up to the end of in_view[point_cap]
        proj[X.PROJ_OFF_VIEW:] = c["in_view"]
        pose = np.full(X.POSE_OFF_OUTLIER + n_kp, 0x5A, np.uint8)   # the pose block up to the end of outlier[n_kp]
        pose[X.POSE_OFF_OUTLIER:] = c["outlier"]
        b.update(proj_out=proj, pose_out=pose, d_out=mr.STAT_OUT_BYTES)
    return b


def extents(c):
    """name -> bytes, by the comments above the declarations in include/spfe.h"""
    nt, rc = len(c["flags"]), len(c["recent"])
    n, stride = c["rows"].shape
    e = dict(flags=nt, nobs=4 * nt, found=4 * nt, visible=4 * nt, first_kf=4 * nt, recent=4 * rc, recent_n=4, rows=4 * stride * n, kf_flags=n,
             xyz=12 * nt)
    if c["op"] == "cull":
        e["d_out"] = X.mpcull_offsets(rc, int(c["bad_cap"]))["out_bytes"]
    elif c["op"] == "admit":
        e.update(tri=int(c["n_neigh"]) * X.tri_offsets(int(c["kmax"]))["out_bytes"], neigh_slot=4 * int(c["n_neigh"]), d_out=X.ADMIT_OUT_BYTES)
    else:
        n_kp, cap = len(c["entry"]), len(c["point_idx"])
        e.update(entry=4 * n_kp, after=4 * n_kp, point_idx=4 * cap, proj_out=X.PROJ_OFF_VIEW + cap, pose_out=X.POSE_OFF_OUTLIER + n_kp,
                 d_out=X.MPSTAT_OUT_BYTES)
    return e


def outputs(c):
    """the buffers the case's call may write"""
    return {"cull": ("rows",) + mr.STATE + ("d_out",), "admit": ("rows", "xyz") + mr.STATE + ("d_out",),
            "stat": ("found", "visible", "d_out")}[c["op"]]


def call(ext, P, c, stream=None):
    """the case's resident form on the addresses P[name] (None / missing = null): nothing is read back, no tensor is made"""
    life = X.mp_life({k: P.get(k) for k in mr.STATE}, len(c["flags"]), len(c["recent"]))
    n, stride = c["rows"].shape
    if c["op"] == "cull":
        ext.cull_map_points_resident(life, P["rows"], stride, P["kf_flags"], n, int(c["cur_kf_id"]), P["d_out"], th_obs=int(c["th_obs"]),
                                     found_ratio=float(np.float32(c["found_ratio"])), bad_cap=int(c["bad_cap"]), stream=stream)
    elif c["op"] == "admit":
        assert ext.layout.kmax == int(c["kmax"]), "the case's blocks are laid out for another handle"
        ext.admit_map_points_resident(life, P["tri"], int(c["n_neigh"]), P["neigh_slot"], int(c["cur_slot"]), int(c["cur_kf_id"]), P["rows"],
                                      stride, n, P["xyz"], P["d_out"], stream=stream)
    else:
        ext.track_statistics_resident(life, P.get("entry"), P.get("after"), len(c["entry"]), P["point_idx"], len(c["point_idx"]),
                                      P["proj_out"], P["pose_out"], P["d_out"], stream=stream)


def want_of(ref, c):
    """the reference's bytes of every output buffer of the case"""
    w, r = mc.run_ref(ref, c)
    want = {k: raw(w[k]) for k in outputs(c) if k != "d_out"}
    want["d_out"] = r["block"]
    return want, r


def run_resident(ext, c, shift=0, stream=None):
    """the resident form on fresh device buffers (the rows `shift` bytes off a 256-byte boundary), the block and a guard behind it
    filled with FILL -> name -> bytes of every output; the guard is checked"""
    import torch
    tens, P = {}, {}
    for k, v in buffers(c).items():
        if isinstance(v, (int, np.integer)):
            t = torch.full((int(v) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        else:
            off = shift if k == "rows" else 0
            t = torch.zeros(off + max(raw(v).size, 16), dtype=torch.uint8, device="cuda")
            if raw(v).size:
                t[off:off + raw(v).size] = torch.from_numpy(raw(v).copy()).cuda()
            t = t[off:]
        tens[k], P[k] = t, t.data_ptr()
    call(ext, P, c, stream)
    torch.cuda.synchronize()
    sizes = buffers(c)
    got = {}
    for k in outputs(c):
        nb = int(sizes[k]) if isinstance(sizes[k], (int, np.integer)) else raw(sizes[k]).size
        host = tens[k].cpu().numpy()
        got[k] = host[:nb].copy()
        if k == "d_out":
            assert (host[nb:] == FILL).all(), "bytes behind the block were written"
    return got


def run_host(ext, c):
    """the host-array form on a copy -> name -> bytes of every output"""
    w = mr.copy_world(c)
    state = {k: w[k] for k in mr.STATE}
    if c["op"] == "cull":
        block = ext.cull_map_points(state, w["rows"], w["kf_flags"], int(c["cur_kf_id"]), th_obs=int(c["th_obs"]),
                                    found_ratio=float(np.float32(c["found_ratio"])), bad_cap=int(c["bad_cap"]), fill=FILL)
    elif c["op"] == "admit":
        block = ext.admit_map_points(state, c["tri"], int(c["n_neigh"]), c["neigh_slot"], int(c["cur_slot"]), int(c["cur_kf_id"]), w["rows"],
                                     w["xyz"], fill=FILL)
    else:
        block = ext.track_statistics(state, c["entry"], c["after"], c["point_idx"], c["in_view"], c["outlier"], fill=FILL)
    got = {k: raw(w[k]) for k in outputs(c) if k != "d_out"}
    got["d_out"] = block
    return got


def same(got, want, c, what):
    for k in outputs(c):
        g, r = np.asarray(got[k]), np.asarray(want[k])
        assert len(g) == len(r), (what, k, len(g), len(r))
        if g.tobytes() != r.tobytes():
            if k == "d_out" and c["op"] == "cull":
                cap, bc = len(c["recent"]), int(c["bad_cap"])
                dg, dr = mr.decode_cull(g, cap, bc), mr.decode_cull(r, cap, bc)
                for f in mr.CULL_FIELDS:
                    assert dg[f] == dr[f], (what, f, dg[f], dr[f])
                for f in ("entry_point", "entry_code", "bad_point"):
                    bad = np.flatnonzero(dg[f] != dr[f])[:8]
                    assert not len(bad), (what, f, bad.tolist(), dg[f][bad].tolist(), dr[f][bad].tolist())
            view = (lambda a: a) if k in ("flags", "kf_flags", "d_out") else (lambda a: a.view(np.int32))
            bad = np.flatnonzero(view(g) != view(r))[:8]
            assert False, (what, k, bad.tolist(), view(g)[bad].tolist(), view(r)[bad].tolist())


def check(ext, ref, c, shift=0, host=True, what=""):
    """one call through mpcull_ref.c, the resident form and (host) the host-array form, all from copies of the case's world -> the
    reference's result"""
    want, r = want_of(ref, c)
    same(run_resident(ext, c, shift), want, c, what + ", resident form")
    if host:
        same(run_host(ext, c), want, c, what + ", host form")
    return r
