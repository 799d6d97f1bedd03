"""What the GPU tests of keyframe culling share: a world on the device, one call through each form of the library, and the
comparison of the block and of everything the call may edit with cull_ref.c byte for byte.  torch is imported inside the
functions."""
import numpy as np

import cull_ref

from sp_orb_slam_amd import extractor as X

FILL = cull_ref.FILL
GUARD = 1024          # bytes behind the block that must keep the preset
POISON = 0x5A         # the bytes of every graph row the call neither reads nor writes
ROWS4 = ("conn_slot", "conn_w", "ord_slot", "ord_w")


def dev(a, shift=0):
    """the array's bytes on the device, `shift` bytes behind a 256-byte boundary"""
    import torch
    a = np.ascontiguousarray(a)
    raw = a.reshape(-1).view(np.uint8)
    t = torch.zeros(shift + max(len(raw), 16), dtype=torch.uint8, device="cuda")
    if len(raw):
        t[shift:shift + len(raw)] = torch.from_numpy(raw.copy()).cuda()
    return t[shift:]


def back(t, like):
    raw = t.cpu().numpy()[:like.nbytes]
    return raw.view(like.dtype).reshape(like.shape).copy()


class DeviceWorld:
    """every array of a world on the device (the rows `shift` bytes off a 256-byte boundary), and the spfe_covis_graph"""

    def __init__(self, w, shift=0):
        self.like = {k: w[k] for k in cull_ref.WORLD if w[k] is not None}
        self.t = {k: dev(v, shift if k == "rows" else 0) for k, v in self.like.items()}
        self.n, self.cap = w["conn_slot"].shape
        self.stride, self.n_table = w["rows"].shape[1], len(w["mp_flags"])
        self.graph = X.covis_graph({k: self.t[k].data_ptr() for k in cull_ref.STATE}, self.n, self.cap)

    def ptr(self, k):
        return self.t[k].data_ptr() if k in self.t and self.like[k].size else None

    def download(self):
        return {k: (back(self.t[k], self.like[k]) if k in self.t else None) for k in cull_ref.WORLD}

    def cull(self, ext, d_out, prm, stream=None):
        ext.cull_keyframes_resident(self.graph, self.ptr("rows"), self.stride, self.ptr("kf_flags"), self.ptr("mp_flags"), self.ptr("nobs"),
                                    self.n_table, prm["cur"], d_out, th_obs=prm["th_obs"], cov_ratio=prm["cov_ratio"],
                                    origin_slot=prm["origin_slot"], bad_cap=prm["bad_cap"], d_best_cov_a=self.ptr("best_a"),
                                    n_best_a=1 if "best_a" not in self.t else self.like["best_a"].shape[1],
                                    d_best_cov_b=self.ptr("best_b"),
                                    n_best_b=1 if "best_b" not in self.t else self.like["best_b"].shape[1], stream=stream)


def run_resident(ext, w, prm, shift=0, stream=None):
    """spfe_cull_keyframes_resident on a copy of the world on the device, the block and a guard behind it filled with FILL ->
    (block, world) as they come back; the guard is checked"""
    import torch
    d = DeviceWorld(w, shift)
    nb = ext.cull_out_bytes(d.n, d.cap, prm["bad_cap"])
    d_out = torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    d.cull(ext, d_out.data_ptr(), prm, stream)
    torch.cuda.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[nb:] == FILL).all(), "bytes behind the block were written"
    return raw[:nb], d.download()


def run_host(ext, w, prm):
    """spfe_cull_keyframes on a copy -> (block, world)"""
    c = cull_ref.copy_world(w)
    block = ext.cull_keyframes({k: c[k] for k in cull_ref.STATE}, c["rows"], c["kf_flags"], c["mp_flags"], c["nobs"], prm["cur"],
                               th_obs=prm["th_obs"], cov_ratio=prm["cov_ratio"], origin_slot=prm["origin_slot"], bad_cap=prm["bad_cap"],
                               best_cov_a=c["best_a"], best_cov_b=c["best_b"], fill=FILL)
    return block, c


def same(got, want, prm, what):
    """(block, world) of a form against the reference's"""
    block, w = got
    wblock, ww = want
    n, cap = ww["conn_slot"].shape
    if block.tobytes() != wblock.tobytes():
        g, r = cull_ref.decode(block, n, cap, prm["bad_cap"]), cull_ref.decode(wblock, n, cap, prm["bad_cap"])
        for k in cull_ref.FIELDS:
            assert g[k] == r[k], (what, k, g[k], r[k])
        for k in r:
            if isinstance(r[k], np.ndarray):
                bad = np.flatnonzero(g[k] != r[k])[:8]
                assert not len(bad), (what, k, bad.tolist(), g[k][bad].tolist(), r[k][bad].tolist())
        assert False, (what, "bytes the block does not name", np.flatnonzero(block != wblock)[:8])
    for k in cull_ref.WORLD:
        if ww[k] is None:
            assert w[k] is None
        elif w[k].tobytes() != ww[k].tobytes():
            bad = np.argwhere(w[k] != ww[k])[:6]
            assert False, (what, k, bad.tolist(), [(w[k][tuple(i)], ww[k][tuple(i)]) for i in bad])


def poison_unread(w, probe_before, probe_after, r, cur):
    """the four graph rows of every slot the call neither reads nor writes filled with POISON: cur, the culled, the keys of their
    maps, the touched, and every slot that has or gets a culled keyframe as its parent keep theirs"""
    n = len(w["kf_flags"])
    keep = np.zeros(n, bool)
    keep[cur] = True
    culled = r["culled_slot"][:r["n_culled"]]
    keep[culled] = True
    keep[r["touched_slot"][:r["n_touched"]]] = True
    for c in culled:
        keys = probe_before["conn_slot"][c, :max(0, int(probe_before["conn_n"][c]))]
        keep[keys[(keys >= 0) & (keys < n)]] = True
    keep |= np.isin(probe_before["parent"], culled) | np.isin(probe_after["parent"], culled)
    ev = r["event_child"][:r["n_events"]]
    keep[ev[(ev >= 0) & (ev < n)]] = True
    for k in ROWS4:
        w[k].view(np.uint8).reshape(n, -1)[~keep] = POISON
    return int((~keep).sum())


def check(ext, ref, w, prm, shift=0, host=True, poison=True, what=""):
    """one call through cull_ref.c, the resident form and (host) the host-array form, all from copies of w; the tables and the block
    hold FILL before the call, and with poison the graph rows of the slots the call has no business with hold POISON before and
    after.  -> (the reference's decoded block, its world)"""
    w = cull_ref.copy_world(w)
    if poison:
        probe = cull_ref.copy_world(w)
        r0 = cull_ref.cull(ref, probe, **prm)
        poison_unread(w, w, probe, r0, prm["cur"])
    ww = cull_ref.copy_world(w)
    r = cull_ref.cull(ref, ww, **prm)
    if poison:
        assert r["block"].tobytes() == r0["block"].tobytes(), "the poison reached a row the reference reads"
    want = (r["block"], ww)
    same(run_resident(ext, w, prm, shift), want, prm, what + ", resident form")
    if host:
        same(run_host(ext, w, prm), want, prm, what + ", host form")
    return r, ww
