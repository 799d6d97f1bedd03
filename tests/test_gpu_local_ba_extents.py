"""GPU: bundle adjustment held to the buffer extents include/spfe.h documents, as tests/test_gpu_extents.py holds the older
forms: spfe_local_ba_records_device is called (a) with separate torch tensors and (b), (c) with EVERY pointer argument inside
one arena (tests/extent_arena.py) at exactly its documented size, the bytes between the buffers filled with 0xFF, then with
0x80; spfe_bundle_adjust the same way with its host arrays in a numpy arena.  No byte outside a buffer may change and every
output must be byte-identical across the calls.  A second pass puts the poison INTO the edge list (whole triples, and single
fields of others) and into the records' rows at and beyond K: a poisoned edge is skipped, never followed, and the rows beyond K
are never read.  The scene and the problem are test_gpu_local_ba.py's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import extent_arena as ea  # noqa: E402
import test_gpu_local_ba as tb  # noqa: E402
from test_gpu_local_ba import S  # noqa: E402,F401  (the module's scene fixture)

from sp_orb_slam_amd import extractor as X  # noqa: E402

pytestmark = pytest.mark.gpu
INTR = tb.INTR

# argument -> bytes, by the comments above the two declarations in include/spfe.h (section "local mapping: bundle adjustment")
EXTENTS = dict(d_edges=lambda d: 12 * d["E"], d_Tcw=lambda d: 64 * d["n_kf"], d_fixed=lambda d: d["n_kf"], d_xyz=lambda d: 12 * d["n"],
               d_stop=lambda d: 4, d_out=lambda d: X.ba_offsets(d["n_kf"], d["n"], d["E"])["bytes"],
               obs_xy=lambda d: 8 * d["E"], inv_sigma2=lambda d: 8 * d["E"])


def poisoned_edges(edges):
    """whole triples and single fields replaced by the pattern (p None: by -1, which is skipped the same way)"""
    def value(p):
        e = edges.copy()
        fill = -1 if p is None else int(np.array([p] * 4, np.uint8).view(np.int32)[0])
        e[[3, 50, len(e) - 1]] = fill
        e[11, 0] = fill
        e[23, 1] = fill
        e[31, 2] = fill
        return e
    return value


def record_with_poisoned_tail(s, f):
    def value(p):
        raw = s.raw[f].copy()
        if p is not None:
            L, K = s.ext.layout, s.recs[f].K
            for off, row in ((L.off_xy, 8), (L.off_cinv, 8)):
                raw[off + K * row:off + L.kmax * row] = p
        return raw
    return value


def test_local_ba_records_device(S):  # noqa: F811
    import torch
    e = S.ext
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    d = dict(n_kf=n_kf, n=n, E=E)
    spec = {"d_record_%d" % f: record_with_poisoned_tail(S, f) for f in range(n_kf)}
    spec.update(d_edges=poisoned_edges(S.edges), d_Tcw=S.Tcw, d_fixed=S.fixed, d_xyz=S.xyz, d_stop=np.zeros(1, np.int32),
                d_out=X.ba_offsets(n_kf, n, E)["bytes"])
    plain = lambda v: v(None) if callable(v) else v   # noqa: E731

    def call(P):
        e.local_ba_records_device([P["d_record_%d" % f] for f in range(n_kf)], P["d_edges"], E, P["d_Tcw"], P["d_fixed"], P["d_xyz"], n,
                                  P["d_out"], INTR, d_stop=P["d_stop"])
        torch.cuda.synchronize()
    tens = {}
    for name, v in spec.items():
        v = plain(v)
        tens[name] = torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else \
            torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()
    call({k: t.data_ptr() for k, t in tens.items()})
    want = {"d_out": tens["d_out"].cpu().numpy()}
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, plain(v), init=0xA5)
        size = S.rb if name.startswith("d_record_") else EXTENTS[name](d)
        assert arena.size(name) == size, (name, arena.size(name), size)
    run = lambda a: call({k: a.ptr(k) for k in spec})   # noqa: E731
    found, got = ea.report(arena, run, ("d_out",), want)
    assert found == [], found

    def tails(a, p):
        for name, v in spec.items():
            if callable(v):
                a.set_initial(name, v(p))
    found, got = ea.report(arena, run, ("d_out",), want, before_fill=tails)
    assert found == [], ("poison in the edges and beyond K", found)
    g = X.SPExtractor.decode_ba_out(got["d_out"], n_kf, n, E)
    assert (g["verdict"][[3, 11, 23, 31, 50, E - 1]] == X.BA_SKIPPED).all() and g["n_served"] == E - 6 and g["iterations"][0] > 0
    assert (got["d_out"][48:64] == 0xA5).all()
    # the inputs are inputs
    for name in ("d_Tcw", "d_fixed", "d_xyz", "d_stop"):
        assert arena.read(name).tobytes() == np.ascontiguousarray(spec[name]).tobytes(), name


def test_local_ba_records_device_with_too_many_free_keyframes(S):  # noqa: F811
    """70 keyframe slots on the six records, 65 flags at 0: the refusal on the device writes the echo and the header inside
    d_out and nothing else, whatever lies around the buffers"""
    import torch
    e = S.ext
    n, E, n_kf = len(S.xyz), len(S.edges), 70
    d = dict(n_kf=n_kf, n=n, E=E)
    Tcw = np.tile(S.Tcw, (12, 1))[:n_kf].copy()
    fixed = np.r_[S.fixed, np.zeros(61, np.uint8), np.ones(3, np.uint8)]
    assert int((fixed == 0).sum()) == X.BA_MAX_FREE + 1
    spec = {"d_record_%d" % f: S.raw[f] for f in range(6)}
    spec.update(d_edges=S.edges, d_Tcw=Tcw, d_fixed=fixed, d_xyz=S.xyz, d_stop=np.zeros(1, np.int32), d_out=X.ba_offsets(n_kf, n, E)["bytes"])
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == (S.rb if name.startswith("d_record_") else EXTENTS[name](d)), name

    def run(a):
        e.local_ba_records_device([a.ptr("d_record_%d" % (f % 6)) for f in range(n_kf)], a.ptr("d_edges"), E, a.ptr("d_Tcw"),
                                  a.ptr("d_fixed"), a.ptr("d_xyz"), n, a.ptr("d_out"), INTR, d_stop=a.ptr("d_stop"))
        torch.cuda.synchronize()
    found, got = ea.report(arena, run, ("d_out",))
    assert found == [], found
    g = X.SPExtractor.decode_ba_out(got["d_out"], n_kf, n, E)
    assert g["status"] == X.BA_STATUS_TOO_MANY_FREE and g["n_free"] == 65 and g["n_served"] == 0 and (g["verdict"] == X.BA_SKIPPED).all()
    assert g["Tcw_out"].tobytes() == Tcw.tobytes() and g["xyz_out"].tobytes() == S.xyz.tobytes() and (got["d_out"][48:64] == 0xA5).all()


def test_bundle_adjust_host_form(S):  # noqa: F811
    e = S.ext
    n_kf, n, E = len(S.Tcw), len(S.xyz), len(S.edges)
    d = dict(n_kf=n_kf, n=n, E=E)
    edges = poisoned_edges(S.edges)
    spec = dict(d_edges=edges, obs_xy=S.obs, inv_sigma2=S.w, d_Tcw=S.Tcw, d_fixed=S.fixed, d_xyz=S.xyz, d_stop=np.zeros(1, np.int32),
                d_out=X.ba_offsets(n_kf, n, E)["bytes"])
    plain = lambda v: v(None) if callable(v) else v   # noqa: E731
    want = {"d_out": e.bundle_adjust(edges(None), S.obs, S.w, S.Tcw, S.fixed, S.xyz, INTR, stop=0, fill=0xA5)}
    arena = ea.Arena("numpy")
    for name, v in spec.items():
        arena.place(name, plain(v), init=0xA5)
        assert arena.size(name) == EXTENTS[name](d), name
    prm = e._ba_params(INTR, X.BA_LOCAL, (5, 10), 1, 1.0)

    def run(a):
        import ctypes as C
        rc = e._lib.spfe_bundle_adjust(e._h, a.ptr("d_edges"), a.ptr("obs_xy"), a.ptr("inv_sigma2"), E, a.ptr("d_Tcw"), a.ptr("d_fixed"),
                                       n_kf, a.ptr("d_xyz"), n, C.byref(prm), a.ptr("d_stop"), a.ptr("d_out"))
        assert rc == 0

    def tails(a, p):
        a.set_initial("d_edges", edges(p))
    found, got = ea.report(arena, run, ("d_out",), want, before_fill=tails)
    assert found == [], found
    g = X.SPExtractor.decode_ba_out(got["d_out"], n_kf, n, E)
    assert (g["verdict"][[3, 11, 23, 31, 50, E - 1]] == X.BA_SKIPPED).all() and g["n_served"] == E - 6
    for name in ("obs_xy", "inv_sigma2", "d_Tcw", "d_fixed", "d_xyz", "d_stop"):
        assert arena.read(name).tobytes() == np.ascontiguousarray(spec[name]).tobytes(), name
