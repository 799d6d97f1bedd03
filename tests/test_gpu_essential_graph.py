"""GPU: the essential graph over Sim3 and the map corrections (spfe_optimize_essential_graph*, spfe_essential_graph_sim3*,
spfe_correct_map_points*; sp_orb_slam_amd/csrc/essgraph.hip) against their host statement tests/eg_ref/eg_ref.c, both built on
include/spfe_essgraph_math.h.

Host form, on every fixture tests/golden/essgraph_*.npz and on the generated cases of tests/eg_ref/eg_cases.py — large (1000
keyframes, ~4500 edges, one loop of 8 x 8 kind-0 connections, 1 % noise), threads (255 ... 1025 unknowns: either side of the
tree's 256 slots, of the workgroup's 512 threads and of twice that), wide_row (one row whose envelope spans all 600 unknowns, a
band of 2 elsewhere), lds_edge (a column panel of capacity - 1, capacity and capacity + 1 block rows) and repeated_pair (one
pair's edge 2000 times: adjacency lists over several chunks of the list build): every integer equal,
Sim3, Tiw and the chi2 values within 4 times the deviation measured on an MI355X.
Measured on an MI355X (ROCm 7, gfx950): MEASURED_DEV = 0.0 on every case: the blocks are equal byte for byte, chi2 and lambda
included.  The contract calls no libm function (its log, acos, sin, cos and exp are the header's own, + - * / sqrt alone;
DESIGN.md 9.16 says why), so a ROCm whose libm differs in a last bit does not move a trial count here.

Device form: the same bytes as the host form on a non-default stream, with every byte of the block that is not named left as
filled.  Refusals leave the outputs untouched.  spfe_essential_graph_sim3_device runs on an optimise block the handle itself
produced (spfe_optimize_sim3 on the fixture tests/golden/sim3opt_clean.npz) and its corrected Sim3, narrowed as
spfe_s3o_sim_to_f32 narrows, equals the d_Siw of spfe_loop_corrected_poses_device bit for bit.  spfe_correct_map_points_device
is compared with the reference on 5000 rows under a shuffled point_idx with every code and NaN rows.  The two chains of
include/spfe.h, each ending in spfe_refresh_map_points_device(SPFE_MP_NORMAL_DEPTH) — the second with d_Tcw = the block's Tiw —
run on one stream on 64 keyframe records with 3000 table rows and give, bit for bit, the xyz, normal, dist_range and codes of the
same steps through the host forms."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "eg_ref", "mp_ref", "golden"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import eg_cases  # noqa: E402
import eg_ref  # noqa: E402
import mp_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W, NF = 128, 160, 100
FILL = 0xA5
MEASURED_DEV = 0.0
BOUND = 4 * MEASURED_DEV


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return eg_ref.build(tmp_path_factory.mktemp("eg_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(NF, H, W, weights.synthetic(7, "dense"), with_heat=False)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "essgraph_%s.npz" % name)))


def cap_of(case):
    a = eg_ref.arrays(case)
    return eg_ref.env_cap_of(case) if "env_cap" in case else SPExtractor.essential_graph_envelope(a["flags"], a["edges"])[0]


def sim_to_f32(S):
    """spfe_s3o_sim_to_f32 / spfe_eg_recover in numpy, operation for operation -> (Siw, Tiw) f32 [16]"""
    q = [float(v) for v in S[:4]]
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    R = [1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)]
    s, inv = float(S[7]), 1.0 / float(S[7])
    A, B = np.zeros(16, np.float32), np.zeros(16, np.float32)
    for r in range(3):
        for c in range(3):
            A[4 * r + c] = np.float32(s * R[3 * r + c])
            B[4 * r + c] = np.float32(R[3 * r + c])
        A[4 * r + 3] = np.float32(float(S[4 + r]))
        B[4 * r + 3] = np.float32(float(S[4 + r]) * inv)
    A[15] = B[15] = 1.0
    return A, B


def same(got_block, want, n, what):
    """the raw block against the reference's result -> the largest deviation of a Sim3 entry"""
    got = SPExtractor.decode_essgraph_out(got_block, n)
    assert [got[k] for k in X.ESSGRAPH_FIELDS] == [want[k] for k in eg_ref.INTS], (what, [got[k] for k in X.ESSGRAPH_FIELDS],
                                                                                   [want[k] for k in eg_ref.INTS])
    dv = float(np.abs(got["sim3"] - want["sim3"]).max())
    dt = float(np.abs(got["Tiw"].astype(np.float64) - want["Tiw"].astype(np.float64)).max())
    dc = max(abs(got[k] - want[k]) for k in ("chi2_initial", "chi2_final", "lambda_final"))
    print("%s: ints %s |Sim3 - ref| %.3e |Tiw - ref| %.3e |chi2, lambda - ref| %.3e bytes equal %s" %
          (what, [got[k] for k in X.ESSGRAPH_FIELDS], dv, dt, dc, bytes(got_block) == bytes(want["block"])))
    assert dv <= BOUND and dc <= BOUND * max(1.0, abs(want["chi2_initial"])), (what, dv, dc)
    rounding = 2.0 ** -24 * max(1.0, float(np.abs(want["Tiw"]).max())) if BOUND > 0 else 0.0
    assert dt <= BOUND + rounding, (what, dt)
    # Tiw is the cast of the block's own Sim3, bit for bit, whatever the bound
    for v in range(n):
        assert got["Tiw"][v].view(np.uint32).tolist() == sim_to_f32(got["sim3"][v])[1].view(np.uint32).tolist(), (what, v)
    raw = np.asarray(got_block)
    assert (raw[~eg_ref.named_mask(n)] == FILL).all(), what
    return dv


def host_form(ext, case, env_cap=None, **kw):
    a = eg_ref.arrays(case)
    prm = eg_ref.params_of(case)
    return ext.optimize_essential_graph(a["est"], a["meas"], a["flags"], a["edges"], cap_of(case) if env_cap is None else env_cap,
                                        prm.iterations, prm.fix_scale, prm.lambda_init, fill=FILL, **kw)


def against_reference(ext, ref, case, what):
    want = eg_ref.solve(ref, case, env_cap=cap_of(case), fill=FILL)
    same(host_form(ext, case), want, len(case["flags"]), what)
    return want


@pytest.mark.parametrize("name", eg_cases.SMALL)
def test_host_form_on_every_fixture(ext, ref, name):
    want = against_reference(ext, ref, load(name), name)
    if name == "floating_component":
        assert want["n_solve_failed"] >= 1
    if name == "rejected_trials":
        assert want["rejected"] >= 1 and want["accepted"] >= 1


def test_large(ext, ref):
    c = eg_cases.large()
    want = against_reference(ext, ref, c, "large")
    assert want["n_unknown"] == 999 and want["status"] == eg_ref.OK and (c["edges"][:, 2] == 0).sum() == 64
    assert want["chi2_final"] < 1e-3 * want["chi2_initial"] and want["rejected"] >= 1


@pytest.mark.parametrize("unknowns", (255, 256, 257, 1023, 1025))
def test_threads(ext, ref, unknowns):
    want = against_reference(ext, ref, eg_cases.banded(unknowns), "threads %d" % unknowns)
    assert want["n_unknown"] == unknowns and want["env_blocks"] == 3 * unknowns - 3


def test_wide_row(ext, ref):
    c = eg_cases.banded(600, wide_row=True)
    want = against_reference(ext, ref, c, "wide_row")
    _, nu, first = SPExtractor.essential_graph_envelope(c["flags"], c["edges"])
    assert nu == 600 and first[599] == 0 and (np.arange(600) - first)[:599].max() == 2 and want["env_blocks"] == 3 * 600 - 3 + 597


def test_lds_edge(ext, ref):
    cap = ext.essgraph_lds_panel_capacity()
    assert 16 <= cap <= 400
    for leaves in (cap - 1, cap, cap + 1):   # the panel of block column 0 has that many block rows
        want = against_reference(ext, ref, eg_cases.star(leaves), "lds_edge %d%+d" % (cap, leaves - cap))
        assert want["n_unknown"] == leaves + 1 and want["env_blocks"] == (leaves + 1) * (leaves + 2) // 2


def test_repeated_pair(ext, ref):
    """duplicate edges are legal, whatever their number: the lists are built by rank, their length costs nothing extra"""
    c = eg_cases.repeated_pair()
    want = against_reference(ext, ref, c, "repeated_pair")
    assert want["n_edges_followed"] == len(c["edges"]) > 2000 and want["env_blocks"] == 3 * 40 - 3 and want["n_skipped"] == 0


def device_form(ext, case, stream=None, env_cap=None):
    import torch
    a = eg_ref.arrays(case)
    n, E = len(a["est"]), len(a["edges"])
    prm = eg_ref.params_of(case)
    d = [dev(a[k]) for k in ("est", "meas", "flags")]
    d_e = dev(a["edges"]) if E else None
    out = torch.full((X.essgraph_offsets(n)["out_bytes"],), FILL, dtype=torch.uint8, device="cuda")
    ext.optimize_essential_graph_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, d_e.data_ptr() if E else None, E,
                                        cap_of(case) if env_cap is None else env_cap, out.data_ptr(), prm.iterations, prm.fix_scale,
                                        prm.lambda_init, stream=stream.cuda_stream if stream is not None else None)
    (stream.synchronize() if stream is not None else torch.cuda.synchronize())
    for k, t in zip(("est", "meas", "flags"), d):   # the inputs are inputs
        assert t.cpu().numpy().tobytes() == a[k].tobytes(), k
    return out.cpu().numpy()


@pytest.mark.parametrize("name", ("chain5_loop", "corrected_subset", "floating_component", "only_fixed", "envelope_overflow",
                                  "skipped_edges", "banded_300"))
def test_device_form_gives_the_host_forms_bytes_on_another_stream(ext, name):
    import torch
    case = eg_cases.banded(300, wide_row=True) if name == "banded_300" else load(name)
    s = torch.cuda.Stream()
    got = device_form(ext, case, stream=s)
    want = host_form(ext, case)
    assert bytes(got) == bytes(want)
    assert (got[~eg_ref.named_mask(len(case["flags"]))] == FILL).all()
    assert bytes(device_form(ext, case)) == bytes(want)   # and on the handle's own stream


def test_refusals_leave_the_outputs_untouched(ext):
    import ctypes as C
    c = load("chain5_loop")
    a = eg_ref.arrays(c)
    n, E = len(a["est"]), len(a["edges"])
    out = np.full(X.essgraph_offsets(n)["out_bytes"], FILL, np.uint8)
    L, h = ext._lib, ext._h
    p = lambda v: v.ctypes.data   # noqa: E731

    def call(est=a["est"], meas=a["meas"], flags=a["flags"], n=n, edges=a["edges"], E=E, cap=64, prm=X.EssGraphParams(20, 0, 1e-16), o=out):
        q = lambda v: None if v is None else p(v)   # noqa: E731
        return L.spfe_optimize_essential_graph(h, q(est), q(meas), q(flags), n, q(edges), E, cap, C.byref(prm) if prm is not None else None,
                                               q(o))
    assert call() == 0
    out[:] = FILL
    bad = [dict(n=0), dict(n=X.ESSGRAPH_MAX_KEYFRAMES + 1), dict(E=X.ESSGRAPH_MAX_EDGES + 1), dict(E=-1), dict(cap=X.ESSGRAPH_MAX_BLOCKS + 1),
           dict(cap=-1), dict(prm=X.EssGraphParams(-1, 0, 1e-16)), dict(prm=X.EssGraphParams(20, 0, -1.0)),
           dict(prm=X.EssGraphParams(20, 0, float("nan"))), dict(est=None), dict(meas=None), dict(flags=None), dict(edges=None),
           dict(prm=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert (out == FILL).all(), kw
    assert L.spfe_optimize_essential_graph(None, p(a["est"]), p(a["meas"]), p(a["flags"]), n, p(a["edges"]), E, 64,
                                           C.byref(X.EssGraphParams(20, 0, 1e-16)), p(out)) == -1
    assert call(o=None) == -1
    # the device form: the same checks before any launch
    import torch
    d_out = torch.full((len(out),), FILL, dtype=torch.uint8, device="cuda")
    d = [dev(a[k]) for k in ("est", "meas", "flags", "edges")]
    for kw in (dict(n=0), dict(env_cap=X.ESSGRAPH_MAX_BLOCKS + 1), dict(iterations=-1), dict(E=X.ESSGRAPH_MAX_EDGES + 1)):
        args = dict(n=n, E=E, env_cap=64, iterations=20)
        args.update(kw)
        with pytest.raises(SpfeError):
            ext.optimize_essential_graph_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), args["n"], d[3].data_ptr(), args["E"],
                                                args["env_cap"], d_out.data_ptr(), iterations=args["iterations"])
    with pytest.raises(SpfeError):
        ext.optimize_essential_graph_device(None, d[1].data_ptr(), d[2].data_ptr(), n, d[3].data_ptr(), E, 64, d_out.data_ptr())
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all()
    # the correction: limits, nulls, and a row listed twice (host form)
    xyz = np.ones((4, 3), np.float32)
    keep = xyz.copy()
    code = np.full(3, FILL, np.uint8)
    with pytest.raises(SpfeError, match="twice"):
        ext.correct_map_points(a["est"], a["meas"], [0, 1, 2], [1, 3, 1], xyz, np.ones(4, np.uint8), code=code)
    assert xyz.tobytes() == keep.tobytes() and (code == FILL).all()
    with pytest.raises(SpfeError):
        ext.correct_map_points_device(d[0].data_ptr(), d[1].data_ptr(), 0, d[2].data_ptr(), None, 1, d[0].data_ptr(), d[2].data_ptr(), 1,
                                      d_out.data_ptr())
    with pytest.raises(SpfeError):
        ext.correct_map_points_device(d[0].data_ptr(), d[1].data_ptr(), n, d[2].data_ptr(), None, X.MP_MAX_POINTS + 1, d[0].data_ptr(),
                                      d[2].data_ptr(), 1, d_out.data_ptr())
    with pytest.raises(SpfeError):
        ext.essential_graph_sim3_device(d[0].data_ptr(), d_out.data_ptr(), d[0].data_ptr(), d[0].data_ptr(), None, 0, n, d[0].data_ptr(),
                                        d[1].data_ptr(), n)   # cur_slot == n


def pose_set(seed, n):
    rng = np.random.default_rng(seed)
    Tcw = np.stack([eg_cases.mat_of(eg_cases.sim_of(M)) for M in eg_cases.trajectory(rng, n)]).astype(np.float32)
    return rng, Tcw


def test_sim3_device_on_a_real_optimise_block(ext, ref):
    """S12 is read out of a block spfe_optimize_sim3 wrote on this handle"""
    import torch
    g = dict(np.load(os.path.join(GOLDEN, "sim3opt_clean.npz")))
    v = [float(x) for x in g["intr"]]
    raw, kcap = ext.optimize_sim3(g["kp_xy1"], g["mp1"], g["kp_xy2"], g["mp2"], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], g["T12"],
                                  g["matches12"], v[:4], v[4:], fix_scale=int(g["fix_scale"]), fill=FILL)
    blk = ext.decode_sim3opt_out(raw, kcap)
    assert blk["accepted"] == 1 and blk["n_in"] >= 20
    S12 = blk["S12"]
    n, cur = 40, 33
    rng, Tcw = pose_set(3, n)
    Tcw2 = np.ascontiguousarray(g["Tcw2"], np.float32).reshape(16)
    Twc = np.linalg.inv(Tcw[cur].astype(np.float64)).astype(np.float32)
    conn = np.array([33, 30, 31, 35, 39, 2, -1, n, 17], np.int32)
    d_blk, d_T, d_T2, d_Twc, d_conn = dev(raw), dev(Tcw), dev(Tcw2), dev(Twc), dev(conn)
    est = torch.full((n * 8,), np.nan, dtype=torch.float64, device="cuda")
    meas = torch.full((n * 8,), np.nan, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    ext.essential_graph_sim3_device(d_T.data_ptr(), d_blk.data_ptr(), d_T2.data_ptr(), d_Twc.data_ptr(), d_conn.data_ptr(), len(conn), cur,
                                    est.data_ptr(), meas.data_ptr(), n, stream=s.cuda_stream)
    s.synchronize()
    est, meas = est.cpu().numpy().reshape(n, 8), meas.cpu().numpy().reshape(n, 8)
    h_est, h_meas = SPExtractor.essential_graph_sim3(Tcw, S12, Tcw2, Twc, conn, cur)
    r_est, r_meas = eg_ref.sim3(ref, Tcw, S12, Tcw2, Twc, conn, cur)
    assert est.tobytes() == h_est.tobytes() == r_est.tobytes() and meas.tobytes() == h_meas.tobytes() == r_meas.tobytes()
    listed = [int(x) for x in conn if 0 <= x < n]
    d_Ti = dev(Tcw[listed])
    Siw = torch.zeros(len(listed) * 16, dtype=torch.float32, device="cuda")
    Tic = torch.zeros(len(listed) * 16, dtype=torch.float32, device="cuda")
    ext.loop_corrected_poses_device(d_blk.data_ptr(), d_T2.data_ptr(), d_Twc.data_ptr(), d_Ti.data_ptr(), len(listed), listed.index(cur),
                                    Siw.data_ptr(), Tic.data_ptr())
    torch.cuda.synchronize()
    Siw, Tic = Siw.cpu().numpy().reshape(-1, 16), Tic.cpu().numpy().reshape(-1, 16)
    for k, slot in enumerate(listed):
        A, B = sim_to_f32(est[slot])
        assert A.view(np.uint32).tolist() == Siw[k].view(np.uint32).tolist(), slot
        assert B.view(np.uint32).tolist() == Tic[k].view(np.uint32).tolist(), slot
    others = [x for x in range(n) if x not in listed]
    assert est[others].tobytes() == meas[others].tobytes() and not np.array_equal(est[listed], meas[listed])


def correction_case(seed=5, n_kf=9, n_table=5000):
    rng = np.random.default_rng(seed)
    S_from = np.stack([eg_cases.sim_of(eg_cases.small_motion(rng, 0.5, 2.0, 0.2)) for _ in range(n_kf)])
    S_to = np.stack([eg_cases.sim_of(eg_cases.small_motion(rng, 0.5, 2.0, 0.2)) for _ in range(n_kf)])
    xyz = rng.normal(0, 5, (n_table, 3)).astype(np.float32)
    flags = (rng.random(n_table) < 0.9).astype(np.uint8) | (rng.integers(0, 2, n_table) * 2).astype(np.uint8)
    idx = rng.permutation(n_table)[:n_table * 3 // 4].astype(np.int32)
    ref_slot = rng.integers(0, n_kf, len(idx)).astype(np.int32)
    idx[:4] = [-1, n_table, n_table + 7, -3]
    ref_slot[4:8] = [-1, n_kf, n_kf + 2, -5]
    xyz[idx[8]] = np.nan
    xyz[idx[9], 1] = np.inf
    flags[idx[4:10]] |= 1
    return S_from, S_to, ref_slot, idx, xyz, flags


def test_correct_map_points(ext, ref):
    import torch
    S_from, S_to, ref_slot, idx, xyz, flags = correction_case()
    want_xyz, want_code = eg_ref.correct(ref, S_from, S_to, ref_slot, idx, xyz, flags)
    assert set(want_code.tolist()) == {X.EGC_SKIP_BAD, X.EGC_INVALID, X.EGC_CORRECTED}
    d = [dev(v) for v in (S_from, S_to, ref_slot, idx, xyz, flags)]
    code = torch.full((len(idx),), FILL, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    ext.correct_map_points_device(d[0].data_ptr(), d[1].data_ptr(), len(S_from), d[2].data_ptr(), d[3].data_ptr(), len(idx), d[4].data_ptr(),
                                  d[5].data_ptr(), len(xyz), code.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    got = d[4].cpu().numpy()
    assert got.view(np.uint32).tolist() == want_xyz.view(np.uint32).tolist() and np.array_equal(code.cpu().numpy(), want_code)
    listed = np.zeros(len(xyz), bool)
    listed[idx[(idx >= 0) & (idx < len(xyz))]] = True
    assert got[~listed].tobytes() == xyz[~listed].tobytes() and np.isnan(got[idx[8]]).all()
    skipped = idx[want_code == X.EGC_SKIP_BAD]
    assert got[skipped].tobytes() == xyz[skipped].tobytes()
    # the host form, and point_idx == NULL (row i)
    h = xyz.copy()
    assert np.array_equal(ext.correct_map_points(S_from, S_to, ref_slot, idx, h, flags), want_code)
    assert h.view(np.uint32).tolist() == want_xyz.view(np.uint32).tolist()
    m = 700
    w2, c2 = eg_ref.correct(ref, S_from, S_to, ref_slot[:m], None, xyz, flags)
    h = xyz.copy()
    assert np.array_equal(ext.correct_map_points(S_from, S_to, ref_slot[:m], None, h, flags), c2) and h.tobytes() == w2.tobytes()
    assert h[m:].tobytes() == xyz[m:].tobytes()


def test_both_chains_on_one_stream(ext, tmp_path):
    """64 keyframe records, 3000 table rows: sim3 -> correct(meas, est) -> refresh(NORMAL_DEPTH), then optimise -> correct(est, the
    block's Sim3) -> refresh with d_Tcw = the block's Tiw, all on one stream with nothing uploaded in between, against the same
    steps through the host forms: xyz, normal, dist_range and every code bit for bit"""
    import torch
    mpl = mp_ref.build(tmp_path)
    n, n_table, cur, K = 64, 3000, 63, 20
    rng, Tcw = pose_set(12, n)
    Tcw2 = Tcw[2].reshape(16).copy()
    Twc = np.linalg.inv(Tcw[cur].astype(np.float64)).astype(np.float32)
    S12m = eg_cases.small_motion(rng, 0.03, 0.2, 0.04) @ Tcw[cur].astype(np.float64).reshape(4, 4) @ np.linalg.inv(Tcw[2].astype(np.float64).reshape(4, 4))
    sc = np.cbrt(np.linalg.det(S12m[:3, :3]))
    S12 = np.concatenate([[sc], (S12m[:3, :3] / sc).reshape(-1), S12m[:3, 3]])
    opt = np.full(X.sim3opt_offsets(80)["out_bytes"], FILL, np.uint8)
    opt[X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104] = S12.view(np.uint8)
    conn = np.arange(56, 64, dtype=np.int32)
    xyz = rng.normal(0, 4, (n_table, 3)).astype(np.float32)
    tflags = (rng.random(n_table) < 0.95).astype(np.uint8)
    m = 2500
    idx = rng.permutation(n_table)[:m].astype(np.int32)
    ref_a = rng.integers(56, 64, m).astype(np.int32)      # the first correction: points of the connected keyframes
    ref_b = rng.integers(0, n, m).astype(np.int32)        # behind the graph: every point by its reference keyframe
    flags = np.zeros(n, np.uint8)
    flags[2] = 1
    edges = [(int(a), int(b), 0) for a in (63, 60) for b in (2, 3)] + [(v - 1, v, 1) for v in range(1, n)] + \
            [(v, v + 3, 1) for v in range(0, n - 3, 2)]
    edges = np.asarray(edges, np.int32)
    cap = SPExtractor.essential_graph_envelope(flags, edges)[0]
    # the observations of the listed points: 2 - 4 each, (keyframe slot, keypoint)
    counts = rng.integers(2, 5, m)
    obs_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    E = int(obs_start[-1])
    obs = np.stack([rng.integers(0, n, E), rng.integers(0, K, E)], 1).astype(np.int32)
    kf_flags = np.zeros(n, np.uint8)
    kf_flags[[5, 40]] = 1   # two bad keyframes

    def host_refresh(poses, table_xyz):
        Ow = mp_ref.camera_centres(mpl, np.ascontiguousarray(poses, np.float32).reshape(n, 16))
        normal, dist_range, desc = mp_ref.poisoned_table(m)
        blk = ext.refresh_map_points(obs_start, np.zeros((E, 256), np.float32), ((kf_flags[obs[:, 0]] & 1) == 0).astype(np.uint8),
                                     Ow[obs[:, 0]], Ow[ref_b], table_xyz[idx], tflags[idx], normal, dist_range, desc,
                                     mode=X.MP_NORMAL_DEPTH, fill=FILL)
        return normal, dist_range, SPExtractor.decode_mp_out(blk, m)["code"]

    # the host forms
    h_est, h_meas = SPExtractor.essential_graph_sim3(Tcw, S12, Tcw2, Twc, conn, cur)
    h_xyz = xyz.copy()
    h_code_a = ext.correct_map_points(h_meas, h_est, ref_a, idx, h_xyz, tflags).copy()
    h_na, h_ra, h_ca = host_refresh(Tcw, h_xyz)
    h_blk = ext.optimize_essential_graph(h_est, h_meas, flags, edges, cap, fill=FILL)
    hb = SPExtractor.decode_essgraph_out(h_blk, n)
    assert hb["status"] == X.ESSGRAPH_OK and hb["iterations"] >= 2 and hb["chi2_final"] < hb["chi2_initial"]
    h_code_b = ext.correct_map_points(h_est, hb["sim3"], ref_b, idx, h_xyz, tflags).copy()
    h_nb, h_rb, h_cb = host_refresh(hb["Tiw"], h_xyz)
    # the device chain
    L, rb = ext.layout, ext.record_bytes()
    raw = np.zeros((n, rb), np.uint8)
    for k in range(n):
        raw[k, L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [K, K, 0, 0]
    d_rec = dev(raw)
    d_ptrs = dev(np.array([d_rec.data_ptr() + k * rb for k in range(n)], np.int64))
    s = torch.cuda.Stream()
    q = lambda t: t.data_ptr()   # noqa: E731
    d_T, d_opt, d_T2, d_Twc, d_conn = dev(Tcw), dev(opt), dev(Tcw2), dev(Twc), dev(conn)
    d_xyz, d_tf, d_idx, d_ra, d_rb, d_fl, d_ed = dev(xyz), dev(tflags), dev(idx), dev(ref_a), dev(ref_b), dev(flags), dev(edges)
    d_kf, d_os, d_obs = dev(kf_flags), dev(obs_start), dev(obs)
    tabs = [[dev(t) for t in mp_ref.poisoned_table(n_table)] for _ in range(2)]
    d_mp = [torch.full((ext.mp_out_bytes(m),), FILL, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_est = torch.zeros(n * 8, dtype=torch.float64, device="cuda")
    d_meas = torch.zeros(n * 8, dtype=torch.float64, device="cuda")
    d_ca = torch.zeros(m, dtype=torch.uint8, device="cuda")
    d_cb = torch.zeros(m, dtype=torch.uint8, device="cuda")
    d_blk = torch.full((len(h_blk),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = s.cuda_stream

    def refresh(d_poses, which):
        t = tabs[which]
        ext.refresh_map_points_device(q(d_ptrs), q(d_kf), d_poses, n, q(d_idx), q(d_os), q(d_obs), q(d_rb), m, E, q(d_xyz), q(d_tf), q(t[0]),
                                      q(t[1]), q(t[2]), n_table, q(d_mp[which]), mode=X.MP_NORMAL_DEPTH, stream=st)
    ext.essential_graph_sim3_device(q(d_T), q(d_opt), q(d_T2), q(d_Twc), q(d_conn), len(conn), cur, q(d_est), q(d_meas), n, stream=st)
    ext.correct_map_points_device(q(d_meas), q(d_est), n, q(d_ra), q(d_idx), m, q(d_xyz), q(d_tf), n_table, q(d_ca), stream=st)
    refresh(q(d_T), 0)
    ext.optimize_essential_graph_device(q(d_est), q(d_meas), q(d_fl), n, q(d_ed), len(edges), cap, q(d_blk), stream=st)
    ext.correct_map_points_device(q(d_est), q(d_blk) + X.essgraph_offsets(n)["sim3"], n, q(d_rb), q(d_idx), m, q(d_xyz), q(d_tf), n_table,
                                  q(d_cb), stream=st)
    refresh(q(d_blk) + X.essgraph_offsets(n)["tiw"], 1)
    s.synchronize()
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32).tolist()   # noqa: E731
    assert d_blk.cpu().numpy().tobytes() == h_blk.tobytes()
    assert bits(d_xyz.cpu().numpy()) == bits(h_xyz)
    assert np.array_equal(d_ca.cpu().numpy(), h_code_a) and np.array_equal(d_cb.cpu().numpy(), h_code_b)
    for which, (h_n, h_r, h_c) in enumerate(((h_na, h_ra, h_ca), (h_nb, h_rb, h_cb))):
        g_n, g_r = tabs[which][0].cpu().numpy(), tabs[which][1].cpu().numpy()
        assert bits(g_n[idx]) == bits(h_n) and bits(g_r[idx]) == bits(h_r), which
        assert np.array_equal(SPExtractor.decode_mp_out(d_mp[which].cpu().numpy(), m)["code"], h_c), which
        rest = np.ones(n_table, bool)
        rest[idx] = False
        assert (g_n[rest].view(np.uint8) == FILL).all() and (g_r[rest].view(np.uint8) == FILL).all()
        assert (h_c == X.MP_REFRESHED).sum() > 2000
    assert bits(h_na) != bits(h_nb)   # the second refresh saw the second correction and the block's poses
    assert not np.array_equal(h_xyz, xyz) and (h_code_a == X.EGC_CORRECTED).sum() > 2000
    del d_rec


def test_two_handles_and_a_handle_where_a_destroyed_one_was(ref):
    blob = weights.synthetic(7, "dense")
    cases = {"corrected_subset": load("corrected_subset"), "banded": eg_cases.banded(300, wide_row=True)}
    want = {k: eg_ref.solve(ref, c, env_cap=cap_of(c), fill=FILL) for k, c in cases.items()}
    a = SPExtractor(NF, H, W, blob, with_heat=False)
    assert bytes(host_form(a, cases["banded"])) == bytes(want["banded"]["block"])
    a.close()
    b = SPExtractor(NF, H, W, blob, with_heat=False)
    c = SPExtractor(NF, H, W, blob, with_heat=False)
    try:
        for _ in range(2):
            assert bytes(host_form(b, cases["corrected_subset"])) == bytes(want["corrected_subset"]["block"])
            assert bytes(host_form(c, cases["banded"])) == bytes(want["banded"]["block"])
            assert bytes(host_form(b, cases["banded"])) == bytes(want["banded"]["block"])
            assert bytes(device_form(c, cases["corrected_subset"])) == bytes(want["corrected_subset"]["block"])
    finally:
        b.close()
        c.close()
