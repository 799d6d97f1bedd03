"""What the GPU tests of the covisibility graph share: the state and the inputs on the device, one call through each form of the
library, and the comparison of block, state and tables with covis_ref.c byte for byte.  torch is imported inside the functions."""
import numpy as np

import covis_ref

from sp_orb_slam_amd import extractor as X

FILL = covis_ref.FILL
GUARD = 1024          # bytes behind the block that must keep the preset
POISON = 0xA5         # the bytes of every state row a call must not touch


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
    """the device bytes as an array of like's dtype and shape"""
    raw = t.cpu().numpy()[:like.nbytes]
    return raw.view(like.dtype).reshape(like.shape).copy()


class DeviceGraph:
    """the eight state arrays on the device, and the spfe_covis_graph that names them"""

    def __init__(self, state):
        self.like = {k: state[k] for k in covis_ref.STATE}
        self.t = {k: dev(state[k]) for k in covis_ref.STATE}
        n, cap = state["conn_slot"].shape
        self.n, self.cap = n, cap
        self.graph = X.covis_graph({k: self.t[k].data_ptr() for k in covis_ref.STATE}, n, cap)

    def download(self):
        return {k: back(self.t[k], self.like[k]) for k in covis_ref.STATE}

    def row_ptr(self, name, slot):
        return self.t[name].data_ptr() + 4 * slot * self.cap


def table(n, n_best, fill=FILL):
    if n_best is None:
        return None
    t = np.empty((n, n_best), np.int32)
    t.view(np.uint8)[...] = fill
    return t


def run_resident(ext, rows, kf_flags, mp_flags, state, cur, th, origin_slot, ta, tb, shift=0, stream=None):
    """spfe_update_connections_resident on copies of state and tables on the device, the block and a guard behind it filled with
    FILL -> (block, state, ta, tb) as they come back; the guard and the read-only inputs are checked"""
    import torch
    rows = np.ascontiguousarray(rows, np.int32)
    n, stride = rows.shape
    g = DeviceGraph(state)
    d_rows, d_f, d_m = dev(rows, shift), dev(np.ascontiguousarray(kf_flags, np.uint8)), dev(np.ascontiguousarray(mp_flags, np.uint8))
    d_ta = None if ta is None else dev(ta)
    d_tb = None if tb is None else dev(tb)
    nb = ext.covis_out_bytes(n, g.cap)
    d_out = torch.full((nb + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    before = [t.clone() for t in (d_rows, d_f, d_m)]
    ext.update_connections_resident(g.graph, d_rows.data_ptr(), stride, d_f.data_ptr(), d_m.data_ptr() if len(mp_flags) else None,
                                    len(mp_flags), cur, d_out.data_ptr(), th=th, origin_slot=origin_slot,
                                    d_best_cov_a=None if ta is None else d_ta.data_ptr(), n_best_a=1 if ta is None else ta.shape[1],
                                    d_best_cov_b=None if tb is None else d_tb.data_ptr(), n_best_b=1 if tb is None else tb.shape[1],
                                    stream=stream)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (d_rows, d_f, d_m))), "a read-only input was written"
    raw = d_out.cpu().numpy()
    assert (raw[nb:] == FILL).all(), "bytes behind the block were written"
    return raw[:nb], g.download(), None if ta is None else back(d_ta, ta), None if tb is None else back(d_tb, tb)


def run_host(ext, rows, kf_flags, mp_flags, state, cur, th, origin_slot, ta, tb):
    """spfe_update_connections on copies -> (block, state, ta, tb)"""
    st = covis_ref.copy_state(state)
    a, b = None if ta is None else ta.copy(), None if tb is None else tb.copy()
    block = ext.update_connections(st, rows, kf_flags, mp_flags, cur, th=th, origin_slot=origin_slot, best_cov_a=a, best_cov_b=b,
                                   fill=FILL)
    return block, st, a, b


def same(got, want, what):
    """(block, state, ta, tb) of a form against the reference's"""
    block, state, ta, tb = got
    wblock, wstate, wta, wtb = want
    n, cap = wstate["conn_slot"].shape
    if block.tobytes() != wblock.tobytes():
        g, w = covis_ref.decode(block, n, cap), covis_ref.decode(wblock, n, cap)
        for k in covis_ref.FIELDS:
            assert g[k] == w[k], (what, k, g[k], w[k])
        for k in ("counter", "linked_slot", "linked_code"):
            assert g[k].tobytes() == w[k].tobytes(), (what, k, np.flatnonzero(g[k] != w[k])[:8])
        assert False, (what, "bytes the block does not name", np.flatnonzero(block != wblock)[:8])
    for k in covis_ref.STATE:
        if state[k].tobytes() != wstate[k].tobytes():
            bad = np.argwhere(state[k] != wstate[k])[:6]
            assert False, (what, "state", k, bad.tolist(), [(state[k][tuple(i)], wstate[k][tuple(i)]) for i in bad])
    for name, t, w in (("table a", ta, wta), ("table b", tb, wtb)):
        assert (t is None) == (w is None)
        if t is not None and t.tobytes() != w.tobytes():
            assert False, (what, name, np.argwhere(t != w)[:6].tolist())


def poison_untouched(state, touched):
    """every state row of the slots outside `touched` filled with POISON: a call must leave those bytes alone"""
    n = state["conn_slot"].shape[0]
    keep = np.zeros(n, bool)
    keep[list(touched)] = True
    for k in covis_ref.STATE:
        state[k].view(np.uint8).reshape(n, -1)[~keep] = POISON   # views of a contiguous array: written in place
    return state


def check(ext, ref, rows, kf_flags, mp_flags, state, cur, th=15, origin_slot=-1, n_best_a=20, n_best_b=10, shift=0, host=True,
          poison=True, what=""):
    """one call through covis_ref.c, the resident form and (host) the host-array form, all from copies of `state`; with poison the
    state rows of every slot the call does not touch (all but cur_slot and P) and both tables hold POISON / FILL bytes before the
    call and must hold them after.  -> (the reference's decoded block, its state, ta, tb)"""
    n = len(rows)
    state = covis_ref.copy_state(state)
    if poison:
        probe = covis_ref.update(ref, rows, kf_flags, mp_flags, covis_ref.copy_state(state), cur, th, origin_slot)
        poison_untouched(state, [cur] + probe["linked_slot"][:probe["n_linked"]].tolist())
    ta, tb = table(n, n_best_a), table(n, n_best_b)
    wst, wta, wtb = covis_ref.copy_state(state), None if ta is None else ta.copy(), None if tb is None else tb.copy()
    r = covis_ref.update(ref, rows, kf_flags, mp_flags, wst, cur, th, origin_slot, wta, wtb)
    want = (r["block"], wst, wta, wtb)
    same(run_resident(ext, rows, kf_flags, mp_flags, state, cur, th, origin_slot, ta, tb, shift), want, what + ", resident form")
    if host:
        same(run_host(ext, rows, kf_flags, mp_flags, state, cur, th, origin_slot, ta, tb), want, what + ", host form")
    return r, wst, wta, wtb
