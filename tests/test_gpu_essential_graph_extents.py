"""GPU: the three device forms of the essential graph held to the buffer extents include/spfe.h documents, as
tests/test_gpu_local_ba_extents.py holds bundle adjustment: every pointer argument sits in one arena (tests/extent_arena.py) at
exactly its documented size, the bytes between the buffers filled with 0xFF, then with 0x80.  No byte outside a buffer may
change and every output must be the ordinary call's, byte for byte.  A second pass puts the poison INTO the lists: edges beyond
E do not exist (the edge buffer ends at 12 E), and inside it whole triples and single fields are poisoned — such an edge is
skipped, never followed; poisoned entries of d_conn_slot, d_ref_slot and d_point_idx are negative and never followed either."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "eg_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import eg_cases  # noqa: E402
import eg_ref  # noqa: E402
import extent_arena as ea  # noqa: E402
import test_gpu_essential_graph as tg  # noqa: E402
from test_gpu_essential_graph import ext  # noqa: E402,F401  (the module's handle)

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

# argument -> bytes, by the comments above the declarations in include/spfe.h (section "loop closing: the essential graph")
EXTENTS = dict(d_Scw_est=lambda d: 64 * d["n"], d_Scw_meas=lambda d: 64 * d["n"], d_flags=lambda d: d["n"], d_edges=lambda d: 12 * d["E"],
               d_out=lambda d: X.essgraph_offsets(d["n"])["out_bytes"], d_Tcw=lambda d: 64 * d["n"], d_opt_block=lambda d: d["opt"],
               d_Tcw2=lambda d: 64, d_Twc=lambda d: 64, d_conn_slot=lambda d: 4 * d["n_conn"], d_S_from=lambda d: 64 * d["n_kf"],
               d_S_to=lambda d: 64 * d["n_kf"], d_ref_slot=lambda d: 4 * d["m"], d_point_idx=lambda d: 4 * d["m"],
               d_xyz=lambda d: 12 * d["n_table"], d_tflags=lambda d: d["n_table"], d_code=lambda d: d["m"])


def poison_i32(p):
    return -1 if p is None else int(np.array([p] * 4, np.uint8).view(np.int32)[0])


def run_in_arena(spec, dims, call, outputs, want, poisoned):
    plain = lambda v: v(None) if callable(v) else v   # noqa: E731
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, plain(v), init=0xA5)
        assert arena.size(name) == EXTENTS[name](dims), (name, arena.size(name), EXTENTS[name](dims))
    found, got = ea.report(arena, lambda a: call({k: a.ptr(k) for k in spec}), outputs, want)
    assert found == [], found

    def tails(a, p):
        for name, v in spec.items():
            if callable(v):
                a.set_initial(name, v(p))
    found, got = ea.report(arena, lambda a: call({k: a.ptr(k) for k in spec}), outputs, poisoned, before_fill=tails)
    assert found == [], ("poison inside the lists", found)
    return arena, got


def test_optimize_essential_graph_device(ext):  # noqa: F811
    import torch
    case = eg_cases.banded(70, wide_row=True)
    a = eg_ref.arrays(case)
    n, E = len(a["est"]), len(a["edges"])
    cap = SPExtractor.essential_graph_envelope(a["flags"], a["edges"])[0]

    def edges(p):
        e = a["edges"].copy()
        fill = poison_i32(p)
        e[[5, 40, E - 1]] = fill
        e[11, 0] = fill
        e[23, 1] = fill
        e[31, 2] = fill
        return e
    spec = dict(d_Scw_est=a["est"], d_Scw_meas=a["meas"], d_flags=a["flags"], d_edges=edges, d_out=X.essgraph_offsets(n)["out_bytes"])

    def call(P):
        ext.optimize_essential_graph_device(P["d_Scw_est"], P["d_Scw_meas"], P["d_flags"], n, P["d_edges"], E, cap, P["d_out"], iterations=3)
        torch.cuda.synchronize()
    want = {"d_out": ext.optimize_essential_graph(a["est"], a["meas"], a["flags"], edges(None), cap, iterations=3, fill=0xA5)}
    arena, got = run_in_arena(spec, dict(n=n, E=E), call, ("d_out",), want, want)
    g = SPExtractor.decode_essgraph_out(got["d_out"], n)
    assert g["n_skipped"] == 6 and g["n_edges_followed"] == E - 6 and g["iterations"] == 3 and g["status"] == X.ESSGRAPH_OK
    assert (got["d_out"][~eg_ref.named_mask(n)] == 0xA5).all()
    for name in ("d_Scw_est", "d_Scw_meas", "d_flags"):
        assert arena.read(name).tobytes() == np.ascontiguousarray(spec[name]).tobytes(), name


def test_essential_graph_sim3_device(ext):  # noqa: F811
    import torch
    n, cur = 30, 21
    rng, Tcw = tg.pose_set(4, n)
    S12 = np.concatenate([[1.03], np.eye(3).reshape(-1), [0.1, -0.2, 0.05]])
    opt = np.full(X.sim3opt_offsets(16)["out_bytes"], 0xA5, np.uint8)
    opt[X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104] = S12.view(np.uint8)
    Twc = np.linalg.inv(Tcw[cur].astype(np.float64)).astype(np.float32)

    def conn(p):
        c = np.array([21, 20, 19, 25, 3, 7, 11], np.int32)
        c[[1, 5]] = poison_i32(p)
        return c
    spec = dict(d_Tcw=Tcw, d_opt_block=opt, d_Tcw2=Tcw[4].copy(), d_Twc=Twc, d_conn_slot=conn, d_Scw_est=64 * n, d_Scw_meas=64 * n)

    def call(P):
        ext.essential_graph_sim3_device(P["d_Tcw"], P["d_opt_block"], P["d_Tcw2"], P["d_Twc"], P["d_conn_slot"], 7, cur, P["d_Scw_est"],
                                        P["d_Scw_meas"], n)
        torch.cuda.synchronize()
    est, meas = SPExtractor.essential_graph_sim3(Tcw, S12, Tcw[4], Twc, conn(None), cur)
    want = {"d_Scw_est": est, "d_Scw_meas": meas}
    run_in_arena(spec, dict(n=n, n_conn=7, opt=len(opt)), call, ("d_Scw_est", "d_Scw_meas"), want, want)
    assert est[20].tobytes() == meas[20].tobytes() and est[19].tobytes() != meas[19].tobytes()


def test_correct_map_points_device(ext, tmp_path):  # noqa: F811
    import torch
    ref = eg_ref.build(tmp_path)
    S_from, S_to, ref_slot, idx, xyz, flags = tg.correction_case(seed=8, n_kf=6, n_table=900)
    m = len(idx)

    def slots(p):
        r = ref_slot.copy()
        r[[20, 300, m - 1]] = poison_i32(p)
        return r

    def rows(p):
        i = idx.copy()
        i[[33, 150, m - 2]] = poison_i32(p)
        return i
    spec = dict(d_S_from=S_from, d_S_to=S_to, d_ref_slot=slots, d_point_idx=rows, d_xyz=xyz, d_tflags=flags, d_code=m)

    def call(P):
        ext.correct_map_points_device(P["d_S_from"], P["d_S_to"], len(S_from), P["d_ref_slot"], P["d_point_idx"], m, P["d_xyz"],
                                      P["d_tflags"], len(xyz), P["d_code"])
        torch.cuda.synchronize()
    w_xyz, w_code = eg_ref.correct(ref, S_from, S_to, slots(None), rows(None), xyz, flags)
    want = {"d_xyz": w_xyz, "d_code": w_code}
    run_in_arena(spec, dict(n_kf=len(S_from), m=m, n_table=len(xyz)), call, ("d_xyz", "d_code"), want, want)
    assert (w_code[[33, 150, m - 2]] == X.EGC_INVALID).all()
