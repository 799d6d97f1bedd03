"""What the GPU tests of the new-keyframe forms share: the buffers of a case (newkf_cases) at exactly their documented sizes, one call
through each form of the library on given addresses, and the comparison of the block and of everything the call may edit with
newkf_ref.c byte for byte.  torch is imported inside the functions."""
import numpy as np

import newkf_cases as nc
import newkf_ref as nr

from sp_orb_slam_amd import extractor as X

FILL = nr.FILL
GUARD = 1024          # bytes behind the block that must keep the preset


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def record_of(ext, rec_desc):
    """a keyframe record of the handle's layout that holds the case's descriptor rows and 0x5A everywhere else"""
    rd = np.ascontiguousarray(rec_desc)
    assert (rd.dtype == np.uint16) == bool(ext.desc_bf16), "the case's descriptor rows are for a handle of the other record format"
    assert rd.shape[0] <= ext.layout.kmax
    rec = np.full(ext.layout.bytes, 0x5A, np.uint8)
    rec[ext.layout.off_desc:ext.layout.off_desc + rd.nbytes] = raw(rd)
    return rec


def buffers(ext, c):
    """name -> the array a pointer argument of the case's resident form points at (its initial contents), or the bytes of an output;
    every one at exactly the extent include/spfe.h documents"""
    if c["op"] == "insert":
        b = {k: c[k] for k in ("rows", "kf_flags") + nr.STATE}
        if len(c["frame"]):
            b["frame"] = np.asarray(c["frame"], np.int32)
        if c.get("rec_desc") is not None:
            b["record"] = record_of(ext, c["rec_desc"])
        if c.get("desc_track") is not None:
            b["desc_track"] = c["desc_track"]
        b["d_out"] = nr.insert_offsets(len(c["frame"]), c["rows"].shape[1])["out_bytes"]
    else:
        b = {k: c[k] for k in ("rows", "kf_flags", "ref_slot")}
        if c["point_idx"] is not None and int(c["m"]):
            b["point_idx"] = np.asarray(c["point_idx"], np.int32)[:int(c["m"])]
        b["d_out"] = nr.list_offsets(int(c["m"]), int(c["obs_cap"]))["out_bytes"]
    return b


def extents(ext, c):
    """name -> bytes, by the comments above the declarations in include/spfe.h"""
    n, stride = c["rows"].shape
    nt = len(c["ref_slot"])
    if c["op"] == "insert":
        n_kp = len(c["frame"])
        return dict(rows=4 * stride * n, kf_flags=n, flags=nt, nobs=4 * nt, recent=4 * len(c["recent"]), recent_n=4, frame=4 * n_kp,
                    record=ext.layout.bytes, desc_track=1024 * nt, d_out=X.newkf_offsets(n_kp, stride)["out_bytes"])
    return dict(rows=4 * stride * n, kf_flags=n, ref_slot=4 * nt, point_idx=4 * int(c["m"]),
                d_out=X.listobs_offsets(int(c["m"]), int(c["obs_cap"]))["out_bytes"])


def outputs(c):
    """the buffers the case's call may write"""
    if c["op"] == "insert":
        return ("rows",) + nr.STATE + (("desc_track",) if c.get("desc_track") is not None else ()) + ("d_out",)
    return ("d_out",)


def call(ext, P, c, stream=None):
    """the case's resident form on the addresses P[name] (None / missing = null): nothing is read back, no tensor is made"""
    n, stride = c["rows"].shape
    if c["op"] == "insert":
        life = X.mp_life(dict(flags=P.get("flags"), nobs=P.get("nobs"), recent=P.get("recent"), recent_n=P.get("recent_n")), len(c["flags"]),
                         len(c["recent"]))
        ext.insert_keyframe_resident(life, P.get("frame"), len(c["frame"]), int(c["cur_slot"]), P["rows"], stride, P["kf_flags"], n, P["d_out"],
                                     d_kf_record=P.get("record"), d_desc_track=P.get("desc_track"), stream=stream)
    else:
        ext.list_observations_resident(P.get("point_idx"), int(c["first_row"]), int(c["m"]), P["rows"], stride, P["kf_flags"], n, P["ref_slot"],
                                       len(c["ref_slot"]), int(c["obs_cap"]), P["d_out"], stream=stream)


def want_of(ref, c):
    """the reference's bytes of every output buffer of the case"""
    w, r = nc.run_ref(ref, c)
    want = {k: raw(w[k]) for k in outputs(c) if k != "d_out"}
    want["d_out"] = r["block"]
    return want, r


def run_resident(ext, c, shift=0, stream=None):
    """the resident form on fresh device buffers (the rows `shift` bytes off a 256-byte boundary), the block and a guard behind it
    filled with FILL -> name -> bytes of every output; the guard is checked"""
    import torch
    tens, P = {}, {}
    spec = buffers(ext, c)
    for k, v in spec.items():
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
    got = {}
    for k in outputs(c):
        nb = int(spec[k]) if isinstance(spec[k], (int, np.integer)) else raw(spec[k]).size
        host = tens[k].cpu().numpy()
        got[k] = host[:nb].copy()
        if k == "d_out":
            assert (host[nb:] == FILL).all(), "bytes behind the block were written"
    return got


def run_host(ext, c):
    """the host-array form on a copy -> name -> bytes of every output"""
    w = nr.copy_world(c)
    if c["op"] == "insert":
        rec = record_of(ext, c["rec_desc"]) if c.get("rec_desc") is not None else None
        block = ext.insert_keyframe({k: w[k] for k in nr.STATE}, c["frame"], int(c["cur_slot"]), w["rows"], w["kf_flags"], kf_record=rec,
                                    desc_track=w["desc_track"], fill=FILL)
    else:
        block = ext.list_observations(c["point_idx"], int(c["first_row"]), int(c["m"]), w["rows"], w["kf_flags"], w["ref_slot"], int(c["obs_cap"]),
                                      fill=FILL)
    got = {k: raw(w[k]) for k in outputs(c) if k != "d_out"}
    got["d_out"] = block
    return got


def same(got, want, c, what):
    for k in outputs(c):
        g, r = np.asarray(got[k]), np.asarray(want[k])
        assert len(g) == len(r), (what, k, len(g), len(r))
        if g.tobytes() != r.tobytes():
            if k == "d_out":
                if c["op"] == "insert":
                    dg, dr = (nr.decode_insert(x, len(c["frame"]), c["rows"].shape[1]) for x in (g, r))
                    fields, arrays = nr.INSERT_FIELDS, ("code", "added_point")
                else:
                    dg, dr = (nr.decode_list(x, int(c["m"]), int(c["obs_cap"])) for x in (g, r))
                    fields, arrays = nr.LIST_FIELDS, ("point_idx", "obs_start", "ref_slot", "obs")
                for f in fields:
                    assert dg[f] == dr[f], (what, f, dg[f], dr[f])
                for f in arrays:
                    bad = np.flatnonzero((dg[f] != dr[f]).reshape(len(dg[f]), -1).any(1))[:8]
                    assert not len(bad), (what, f, bad.tolist(), dg[f][bad].tolist(), dr[f][bad].tolist())
            view = (lambda a: a) if k in ("flags", "d_out") else (lambda a: a.view(np.int32))
            bad = np.flatnonzero(view(g) != view(r))[:8]
            assert False, (what, k, bad.tolist(), view(g)[bad].tolist(), view(r)[bad].tolist())


def check(ext, ref, c, shift=0, host=True, what=""):
    """one call through newkf_ref.c, the resident form and (host) the host-array form, all from copies of the case's world -> the
    reference's result"""
    want, r = want_of(ref, c)
    same(run_resident(ext, c, shift), want, c, what + ", resident form")
    if host:
        same(run_host(ext, c), want, c, what + ", host form")
    return r
